// Local (amino-acid) pretraining head + its loss, reference semantics: one launch up to
// 2048 samples per GPU (lhead_onepass_kernel, below), coalesced multi-pass kernels above that and when a
// data-parallel group shares the batch axis of the softmax.
//
// Reference: ProteinBERT/modules.py:277-284,304 (Linear C -> V, then nn.Softmax() with the implicit
// dim, which for the [B, L, V] output is dim 0: a softmax over the BATCH for every (position, token))
// and ProteinBERT/utils.py:293 (CrossEntropyLoss over V applied to those probabilities, times the
// per-residue weight, mean over B * L):
//   Z[b,l,v]  = h[b,l,:] . Wo[v,:] + bo[v]
//   P[b,l,v]  = exp(Z - M[l,v]) / S[l,v],       M = max_b Z, S = sum_b exp(Z - M)
//   loss      = 1/(BL) sum_{b,l} w[b,l] (log sum_v exp(P[b,l,v]) - P[b,l,y])
//   G[b,l,v]  = w/(BL) (exp(P)/se - [v == y])                      (dloss/dP)
//   dZ        = P (G - T[l,v]),  T[l,v] = sum_b G P                 (softmax-over-batch backward)
//   dh = dZ Wo ;  dWo = dZ^T h ;  dbo = sum dZ
//
// The batch coupling needs two statistics per (l, v) over all B samples before any gradient exists,
// so the multi-pass form runs as passes over row tiles of 16 samples x 32 positions (each sample's 32
// rows are one contiguous 8 KB run of h): (1) logits + per-tile (max, sum exp) partials, (2) fold them to
// (M, 1/S), (3) CE loss + per-tile partials of G P, (4) fold them to T, (5) dZ, dh = dZ Wo (MFMA) and dZ
// rows for the dWo GEMM; every pass streams contiguous rows, but Z (fp32) is written once and read twice.
// The one-launch form gives a workgroup one POSITION and all B samples: its rows are 256-B runs L * 256
// bytes apart (the round-2 form of it, one tile in flight, ran at ~150 us for B = L = 512), which it reads
// two tiles ahead per wave, and nothing but h, y, w, dh and dz crosses the memory bus.
#include "mfma.h"

using namespace pbx;
typedef unsigned short bf16_t;

namespace {
constexpr int CH = 128;
constexpr int SB = 16;     // samples per tile
constexpr int PT = 32;     // positions per tile
constexpr int VP = 32;     // padded vocabulary

// Wo (fp32 [V][128]) -> bf16 LDS tile [32][128] (swz256, rows >= V zero); bias into bo_s[32]
__device__ __forceinline__ void stage_wo(unsigned char* wos, float* bo_s, const float* __restrict__ wo,
                                        const float* __restrict__ bo, int V) {
  for (int idx = threadIdx.x; idx < VP * 16; idx += blockDim.x) {
    const int v = idx >> 4, c8 = idx & 15;
    float e[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (v < V) {
      const float4 a = *reinterpret_cast<const float4*>(wo + v * CH + c8 * 8);
      const float4 b = *reinterpret_cast<const float4*>(wo + v * CH + c8 * 8 + 4);
      e[0] = a.x; e[1] = a.y; e[2] = a.z; e[3] = a.w; e[4] = b.x; e[5] = b.y; e[6] = b.z; e[7] = b.w;
    }
    *reinterpret_cast<uint4*>(wos + swz256(v, c8)) = packq8(e);
  }
  if (threadIdx.x < VP) bo_s[threadIdx.x] = threadIdx.x < V ? bo[threadIdx.x] : 0.f;
}

// tile id -> (first sample, first position); tiles ordered position-tile-major within a sample chunk
__device__ __forceinline__ void tile_of(int L, int& b0, int& p0, int& chunk) {
  const int TP = (L + PT - 1) / PT;
  chunk = blockIdx.x / TP;
  b0 = chunk * SB;
  p0 = (blockIdx.x - chunk * TP) * PT;
}

// ---- pass 1: Z = h Wo^T + bo (fp32, [B*L][32]) and per-tile (max, sum exp) over the tile's samples
__global__ void __launch_bounds__(512) lhead_logits_kernel(const bf16_t* __restrict__ h, const float* __restrict__ wo,
                                                           const float* __restrict__ bo, float* __restrict__ Z,
                                                           float2* __restrict__ part, int B, int L, int V) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* wos = smem;                                              // [32][128] bf16
  float* bo_s = reinterpret_cast<float*>(smem + VP * 256);                // [32]
  float (*zt)[PT][VP + 1] = reinterpret_cast<float (*)[PT][VP + 1]>(bo_s + VP);   // [SB][PT][VP + 1]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r = lane & 31, hh = lane >> 5;
  int b0, p0, chunk;
  tile_of(L, b0, p0, chunk);
  stage_wo(wos, bo_s, wo, bo, V);
  __syncthreads();
  bf16x8 wf[8];
#pragma unroll
  for (int kk = 0; kk < 8; ++kk) wf[kk] = lds_frag(wos, swz256(r, kk * 2 + hh));
  const float bv = bo_s[r];
#pragma unroll
  for (int si = 0; si < 2; ++si) {
    const int sl = 2 * w + si, b = b0 + sl;
    const int pos = p0 + r;
    const size_t row = (size_t)min(b, B - 1) * L + min(pos, L - 1);        // clamped: loads in bounds
    bf16x8 hf[8];
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) hf[kk] = *reinterpret_cast<const bf16x8*>(h + row * CH + kk * 16 + 8 * hh);
    f32x16_t acc = zero16();
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) acc = mfma32(hf[kk], wf[kk], acc);
    // D[pos][v]: lane column v = r, rows (e & 3) + 8 (e >> 2) + 4 hh
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int pl = (e & 3) + 8 * (e >> 2) + 4 * hh;
      const int pp = p0 + pl;
      const float z = acc[e] + bv;
      zt[sl][pl][r] = z;
      if (b < B && pp < L) Z[((size_t)b * L + pp) * VP + r] = r < V ? z : 0.f;
    }
  }
  __syncthreads();
  // (max, sum exp) over the tile's valid samples for each (position, v): thread -> (pl, v pair)
  {
    const int pl = tid >> 4, v0 = (tid & 15) * 2;
    const int pp = p0 + pl;
    const int nb = min(SB, B - b0);
    if (pp < L) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int v = v0 + j;
        float m = -3.0e38f;
        for (int s = 0; s < nb; ++s) m = fmaxf(m, zt[s][pl][v]);
        float se = 0.f;
        for (int s = 0; s < nb; ++s) se += __expf(zt[s][pl][v] - m);
        part[((size_t)chunk * L + pp) * VP + v] = make_float2(m, se);
      }
    }
  }
}

// ---- passes 2 / 4: fold the per-chunk partials of every (l, v)
//  mode 0: (max, sum exp) -> (M, 1/S);  mode 1: sum G P -> T (stored in .x)
// 64 (l, v) entries per workgroup, the chunks split over 4 thread groups (one pass with an online
// max / rescaled-sum merge, 4x the loads in flight of a thread walking all chunks twice), the four
// partials combined in a fixed order
__global__ void __launch_bounds__(256) lhead_fold_kernel(const float2* __restrict__ part, int nchunks, int L,
                                                         float2* __restrict__ out, int mode) {
  __shared__ float2 red[4][64];
  const int il = threadIdx.x & 63, cg = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + il;                 // l * 32 + v
  const bool ok = i < L * VP;
  float m = -3.0e38f, sum = 0.f;
  if (ok) {
    for (int c = cg; c < nchunks; c += 4) {
      const float2 p = part[(size_t)c * L * VP + i];
      if (mode != 1) {
        const float mn = fmaxf(m, p.x);
        sum = sum * __expf(m - mn) + p.y * __expf(p.x - mn);
        m = mn;
      } else {
        sum += p.x;
      }
    }
  }
  red[cg][il] = make_float2(m, sum);
  __syncthreads();
  if (cg != 0 || !ok) return;
  if (mode != 1) {
    float mm = red[0][il].x;
#pragma unroll
    for (int k = 1; k < 4; ++k) mm = fmaxf(mm, red[k][il].x);
    float ss = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) ss += red[k][il].y * __expf(red[k][il].x - mm);
    out[i] = make_float2(mm, mode == 2 ? ss : ss > 0.f ? 1.0f / ss : 0.f);   // mode 2: raw (M, S)
  } else {
    out[i] = make_float2(red[0][il].y + red[1][il].y + red[2][il].y + red[3][il].y, 0.f);
  }
}

// Per-lane row math shared by passes 3 and 5: lane (r, hh) owns row (b, pos) and the 16 tokens
// v = 8 hh + j (j < 8) and 16 + 8 hh + j; the two lanes of a row (hh = 0, 1) exchange their halves
// of sum_v exp(P).  Returns P, G for the 16 tokens and the row's CE term (on hh = 0; 0 elsewhere).
struct RowTerms {
  float P[16], G[16];
  float loss;
};
__device__ __forceinline__ RowTerms row_terms(const float* __restrict__ Z, const float2* ms, size_t row, int pl,
                                              int hh, int V, bool ok, int yv, float coef) {
  RowTerms t;
  float zv[16];
  {
    const float4* zp0 = reinterpret_cast<const float4*>(Z + row * VP + 8 * hh);
    const float4* zp1 = reinterpret_cast<const float4*>(Z + row * VP + 16 + 8 * hh);
    const float4 a = zp0[0], b = zp0[1], c = zp1[0], d = zp1[1];
    const float tmp[16] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w, d.x, d.y, d.z, d.w};
#pragma unroll
    for (int j = 0; j < 16; ++j) zv[j] = tmp[j];
  }
  float e[16], se = 0.f, py = 0.f;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int v = (j < 8 ? 0 : 16) + 8 * hh + (j & 7);
    const float2 s = ms[pl * VP + v];
    const bool inv = v < V;
    t.P[j] = inv ? __expf(zv[j] - s.x) * s.y : 0.f;
    e[j] = inv ? __expf(t.P[j]) : 0.f;
    se += e[j];
    py += v == yv ? t.P[j] : 0.f;
  }
  se += __shfl_xor(se, 32, 64);
  const float rse = 1.0f / se;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int v = (j < 8 ? 0 : 16) + 8 * hh + (j & 7);
    t.G[j] = ok ? coef * (e[j] * rse - (v == yv ? 1.f : 0.f)) : 0.f;
  }
  // this lane's share of w (log se - P[y]) (the coefficient w / (B L) is applied by the caller)
  t.loss = ok ? ((hh == 0 ? __logf(se) : 0.f) - py) : 0.f;
  return t;
}

// ---- pass 3: CE loss and per-tile partials of T = sum_b G P
__global__ void __launch_bounds__(512) lhead_ce_kernel(const float* __restrict__ Z, const float2* __restrict__ MS,
                                                       const long long* __restrict__ y, const float* __restrict__ wl,
                                                       float2* __restrict__ tpart, float* __restrict__ loss_part,
                                                       int B, int L, int V, float inv_bl) {
  __shared__ float2 ms[PT * VP];
  __shared__ float gp[8][PT][VP + 1];           // per wave: sum over its 2 samples
  __shared__ float red[8];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r = lane & 31, hh = lane >> 5;
  int b0, p0, chunk;
  tile_of(L, b0, p0, chunk);
  for (int i = tid; i < PT * VP; i += 512) {
    const int pp = min(p0 + i / VP, L - 1);
    ms[i] = MS[(size_t)pp * VP + (i % VP)];
  }
  __syncthreads();
  float acc[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) acc[j] = 0.f;
  float lsum = 0.f;
#pragma unroll
  for (int si = 0; si < 2; ++si) {
    const int b = b0 + 2 * w + si, pos = p0 + r;
    const bool ok = b < B && pos < L;
    const size_t row = (size_t)min(b, B - 1) * L + min(pos, L - 1);
    const int yv = (int)y[row];
    const float wgt = ok ? wl[row] : 0.f;
    const RowTerms t = row_terms(Z, ms, row, r, hh, V, ok, yv, wgt * inv_bl);
    lsum += wgt * t.loss;
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] += t.G[j] * t.P[j];
  }
#pragma unroll
  for (int j = 0; j < 16; ++j) gp[w][r][(j < 8 ? 0 : 16) + 8 * hh + (j & 7)] = acc[j];
  lsum = wave_reduce_sum(lsum);
  if (lane == 0) red[w] = lsum;
  __syncthreads();
  for (int i = tid; i < PT * VP; i += 512) {
    const int pl = i / VP, v = i % VP;
    if (p0 + pl < L) {
      float s = 0.f;
#pragma unroll
      for (int ww = 0; ww < 8; ++ww) s += gp[ww][pl][v];
      tpart[((size_t)chunk * L + p0 + pl) * VP + v] = make_float2(s, 0.f);
    }
  }
  if (tid == 0) {
    float s = 0.f;
#pragma unroll
    for (int ww = 0; ww < 8; ++ww) s += red[ww];
    loss_part[blockIdx.x] = s * inv_bl;
  }
}

// ---- pass 5: dZ = P (G - T), dh = dZ Wo (MFMA), dZ rows (bf16 [B*L][32]) for the dWo GEMM and the
// per-workgroup dbo partials.  Wave w: samples 2w, 2w+1 of the tile.
__global__ void __launch_bounds__(512) lhead_grad_kernel(const float* __restrict__ Z, const float2* __restrict__ MS,
                                                         const float2* __restrict__ T, const long long* __restrict__ y,
                                                         const float* __restrict__ wl, const float* __restrict__ wo,
                                                         const float* __restrict__ bo, bf16_t* __restrict__ dh,
                                                         bf16_t* __restrict__ dz, float* __restrict__ dbo_part, int B,
                                                         int L, int V, float inv_bl) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* ot = smem;                                               // [8 waves][32][128] bf16: dh staging
  unsigned char* wos = smem + 8 * PT * 256;                               // [32][128] bf16
  float2* ms = reinterpret_cast<float2*>(wos + VP * 256);                 // [PT * VP]
  float* ts = reinterpret_cast<float*>(ms + PT * VP);                     // [PT * VP]
  float* bo_s = ts + PT * VP;                                             // [VP]
  float (*dbr)[VP] = reinterpret_cast<float (*)[VP]>(bo_s + VP);          // [8][VP]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r = lane & 31, hh = lane >> 5;
  const int q = tr_q(lane), tc = tr_c(lane);
  int b0, p0, chunk;
  tile_of(L, b0, p0, chunk);
  stage_wo(wos, bo_s, wo, bo, V);
  for (int i = tid; i < PT * VP; i += 512) {
    const int pp = min(p0 + i / VP, L - 1);
    ms[i] = MS[(size_t)pp * VP + (i % VP)];
    ts[i] = T[(size_t)pp * VP + (i % VP)].x;
  }
  __syncthreads();
  float dba[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) dba[j] = 0.f;
  unsigned char* myot = ot + w * PT * 256;
#pragma unroll 1
  for (int si = 0; si < 2; ++si) {
    const int b = b0 + 2 * w + si, pos = p0 + r;
    const bool ok = b < B && pos < L;
    const size_t row = (size_t)min(b, B - 1) * L + min(pos, L - 1);
    const int yv = (int)y[row];
    const float wgt = ok ? wl[row] : 0.f;
    const RowTerms t = row_terms(Z, ms, row, r, hh, V, ok, yv, wgt * inv_bl);
    float d[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int v = (j < 8 ? 0 : 16) + 8 * hh + (j & 7);
      d[j] = ok && v < V ? t.P[j] * (t.G[j] - ts[r * VP + v]) : 0.f;
      dba[j] += d[j];
    }
    const bf16x8 f0 = pack8(d), f1 = pack8(d + 8);      // k-steps 0 / 1: v = 8 hh + j, 16 + 8 hh + j
    if (ok) {
      *reinterpret_cast<bf16x8*>(dz + row * VP + 8 * hh) = f0;
      *reinterpret_cast<bf16x8*>(dz + row * VP + 16 + 8 * hh) = f1;
    }
    // dh[pos][c] = sum_v dZ[pos][v] Wo[v][c]: A = dZ rows (this lane's fragments), B = Wo tile read
    // transposed (K = v along its rows)
    f32x16_t acc[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) acc[ct] = zero16();
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int rlo = kk * 16 + 8 * hh + q;
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const int col = ct * 32 + tc;
        const bf16x8 fb = cat_tr(lds_tr(wos, swz256e(rlo, col)), lds_tr(wos, swz256e(rlo + 4, col)));
        acc[ct] = mfma32(kk == 0 ? f0 : f1, fb, acc[ct]);
      }
    }
    // stage the 32 x 128 bf16 tile (rows (e & 3) + 8 (e >> 2) + 4 hh, column ct * 32 + r), then
    // 256-B row stores
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
      for (int e = 0; e < 16; ++e)
        *reinterpret_cast<bf16_t*>(myot + swz256e((e & 3) + 8 * (e >> 2) + 4 * hh, ct * 32 + r)) = f2bf(acc[ct][e]);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (b < B) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int idx = lane + 64 * i;           // 512 16-B chunks = 32 rows x 16
        const int rr = idx >> 4, c8 = idx & 15;
        if (p0 + rr < L)
          *reinterpret_cast<uint4*>(dh + ((size_t)b * L + p0 + rr) * CH + c8 * 8) =
              *reinterpret_cast<const uint4*>(myot + swz256(rr, c8));
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  // dbo partial: sum over the wave's rows (lanes with the same hh) then over the 8 waves
#pragma unroll
  for (int j = 0; j < 16; ++j) {
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) dba[j] += __shfl_xor(dba[j], o, 64);
  }
  if (r == 0) {
#pragma unroll
    for (int j = 0; j < 16; ++j) dbr[w][(j < 8 ? 0 : 16) + 8 * hh + (j & 7)] = dba[j];
  }
  __syncthreads();
  if (tid < V) {
    float s = 0.f;
#pragma unroll
    for (int ww = 0; ww < 8; ++ww) s += dbr[ww][tid];
    dbo_part[(size_t)blockIdx.x * V + tid] = s;
  }
}

// ---- one-launch form (B <= 2048), the logits in REGISTERS (B <= 256 * TPW; TPW = 2, 4, 8).  A workgroup
// owns one position and ALL samples, so both batch reductions ((max, sum exp), then T = sum_b G P) are
// workgroup-local, the head is one pass over h and Z never leaves the CU.  Wave w owns the 32-sample row
// tiles w, w + 8, ... (TPW of them) and keeps their logits transposed, in the MFMA accumulator layout of
// Z^T = Wo h^T: lane (r, hh) holds sample r of each tile and the 16 tokens v = (e & 3) + 8 (e >> 2) + 4 hh,
// so 2048 x 32 fp32 logits are 128 VGPRs per lane and never touch LDS.  (1) h tiles through a register ring RING tiles deep per wave (loads of tile
// i + RING issued behind the MFMAs of tile i: 8 waves x RING x 8 KB in flight per CU), (2) per-wave
// (max, sum exp) by lane butterflies, merged over the 8 waves -> (M, 1/S); E = exp(Z - m_wave) stays in
// registers and P = E exp(m_wave - M) / S costs no second exp, (3) per sample the CE term and G P, summed
// to T the same way, (4) per tile dZ = P (G - T) (exp(P) recomputed: keeping it would double the
// registers), the bf16 dz rows, dh^T = Wo^T dZ^T (MFMA; K = v in the accumulator's own order, the Wo
// fragment read with the matching row permutation), staged through the wave's LDS tile for 256-B row
// stores that drain behind the next tile's math, (5) dbo partial.  No table, no atomics, no workspace.
constexpr int OP_RING = 2;
constexpr int OP_OTS = 272;      // staging row stride (256 B + 16): column writes / row reads at immediate offsets
// two workgroups fit the 160 KiB of a CU (TPW = 2 leaves the registers for them)
constexpr int OP_LDS = 8 * PT * OP_OTS + VP * 256 + VP * 4 + 8 * VP * 8 + VP * 8 + VP * 4 + 8 * 4;
static_assert(2 * OP_LDS <= 160 * 1024, "two workgroups per CU");

template <int TPW>
__global__ void __launch_bounds__(512) lhead_onepass_kernel(const bf16_t* __restrict__ h, const float* __restrict__ wo,
                                                            const float* __restrict__ bo,
                                                            const long long* __restrict__ y,
                                                            const float* __restrict__ wl, bf16_t* __restrict__ dh,
                                                            bf16_t* __restrict__ dz, float* __restrict__ dbo_part,
                                                            float* __restrict__ loss_part, int B, int L, int V,
                                                            float inv_bl) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* ot = smem;                                                // [8 waves][32][128] bf16: dh staging
  unsigned char* wos = smem + 8 * PT * OP_OTS;                             // [32][128] bf16
  float* bo_s = reinterpret_cast<float*>(wos + VP * 256);                  // [32]
  float2* red = reinterpret_cast<float2*>(bo_s + VP);                      // [8][32] per-wave (max, sum exp)
  float2* ms = red + 8 * VP;                                               // [32] (M, 1/S)
  float* tred = reinterpret_cast<float*>(red);                             // [8][32] per-wave sum G P, then sum dZ
  float* dbr = tred + 8 * VP;                                              //   (each behind a barrier after red's / tred's readers)
  float* tt = reinterpret_cast<float*>(ms + VP);                           // [32] T
  float* lred = tt + VP;                                                   // [8]
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, hh = lane >> 5;
  const int q = tr_q(lane), tc = tr_c(lane);
  const int l = blockIdx.x;
  const int NT = (B + 31) >> 5;
  // (1) logits: Z^T tile = Wo h_tile^T
  bf16x8 ring[OP_RING][8];
  auto load_tile = [&](bf16x8 (&dst)[8], int t) {
    const int s = min(t * 32 + r, B - 1);                                  // clamped: loads in bounds
    const bf16_t* src = h + ((size_t)s * L + l) * CH + 8 * hh;
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) dst[kk] = *reinterpret_cast<const bf16x8*>(src + kk * 16);
  };
#pragma unroll
  for (int i = 0; i < OP_RING && i < TPW; ++i)
    if (w + 8 * i < NT) load_tile(ring[i], w + 8 * i);
  stage_wo(wos, bo_s, wo, bo, V);
  __syncthreads();
  float Z[TPW][16];
  {
    bf16x8 wf[8];
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) wf[kk] = lds_frag(wos, swz256(r, kk * 2 + hh));
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
      const int t = w + 8 * i;
      f32x16_t acc = zero16();
      if (t < NT) {
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) acc = mfma32(wf[kk], ring[i % OP_RING][kk], acc);
        if (i + OP_RING < TPW && t + 8 * OP_RING < NT) load_tile(ring[i % OP_RING], t + 8 * OP_RING);
      }
#pragma unroll
      for (int e = 0; e < 16; ++e) Z[i][e] = acc[e];
    }
  }
  // (2) (max, sum exp) over the samples of every token: in-lane over the tiles, butterfly over the 32
  // samples of a tile row, then over the waves
  float m[16], f[16];
  {
    const float4* bp = reinterpret_cast<const float4*>(bo_s + 4 * hh);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4 b4 = bp[2 * g];
      f[4 * g] = b4.x; f[4 * g + 1] = b4.y; f[4 * g + 2] = b4.z; f[4 * g + 3] = b4.w;
    }
  }
#pragma unroll
  for (int e = 0; e < 16; ++e) m[e] = -3.0e38f;
#pragma unroll
  for (int i = 0; i < TPW; ++i) {
    const bool ok = (w + 8 * i) * 32 + r < B;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      Z[i][e] = ok ? Z[i][e] + f[e] : -3.0e38f;
      m[e] = fmaxf(m[e], Z[i][e]);
    }
  }
#pragma unroll
  for (int e = 0; e < 16; ++e) {
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) m[e] = fmaxf(m[e], __shfl_xor(m[e], o, 64));
  }
#pragma unroll
  for (int e = 0; e < 16; ++e) f[e] = 0.f;
#pragma unroll
  for (int i = 0; i < TPW; ++i) {
    const bool ok = (w + 8 * i) * 32 + r < B;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      Z[i][e] = ok ? __expf(Z[i][e] - m[e]) : 0.f;
      f[e] += Z[i][e];
    }
  }
#pragma unroll
  for (int e = 0; e < 16; ++e) {
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) f[e] += __shfl_xor(f[e], o, 64);
  }
  if (r == 0) {
#pragma unroll
    for (int e = 0; e < 16; ++e) red[w * VP + (e & 3) + 8 * (e >> 2) + 4 * hh] = make_float2(m[e], f[e]);
  }
  // labels and weights of this lane's samples (clamped addresses, loaded unconditionally: in flight
  // behind the merge over the waves)
  int yv[TPW];
  float wg[TPW];
#pragma unroll
  for (int i = 0; i < TPW; ++i) {
    const int s = (w + 8 * i) * 32 + r;
    const size_t gi = (size_t)min(s, B - 1) * L + l;
    const long long yr = y[gi];
    const float wr = wl[gi];
    yv[i] = s < B ? (int)yr : -1;
    wg[i] = s < B ? wr : 0.f;
  }
  __syncthreads();
  if (tid < VP) {
    float mm = red[tid].x;
#pragma unroll
    for (int k = 1; k < 8; ++k) mm = fmaxf(mm, red[k * VP + tid].x);
    float ss = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) ss += red[k * VP + tid].y * __expf(red[k * VP + tid].x - mm);
    ms[tid] = make_float2(mm, tid < V && ss > 0.f ? 1.0f / ss : 0.f);
  }
  __syncthreads();
  // P = E exp(m_wave - M) / S (0 for v >= V and for rows past B)
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const float2 mv = ms[(e & 3) + 8 * (e >> 2) + 4 * hh];
    f[e] = __expf(m[e] - mv.x) * mv.y;
  }
#pragma unroll
  for (int i = 0; i < TPW; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) Z[i][e] *= f[e];
  // (3) per sample: CE term and G P
  float lse[TPW], lsum = 0.f;
#pragma unroll
  for (int e = 0; e < 16; ++e) f[e] = 0.f;
#pragma unroll
  for (int i = 0; i < TPW; ++i) {
    float ex[16], se = 0.f, py = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int v = (e & 3) + 8 * (e >> 2) + 4 * hh;
      ex[e] = v < V ? __expf(Z[i][e]) : 0.f;
      se += ex[e];
      py += v == yv[i] ? Z[i][e] : 0.f;
    }
    se += __shfl_xor(se, 32, 64);
    const float rse = 1.0f / se;                       // se >= V: exp(P) >= 1 for every v < V
    lse[i] = __logf(se);
    const float coef = wg[i] * inv_bl;
    lsum += wg[i] * ((hh == 0 ? lse[i] : 0.f) - py);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int v = (e & 3) + 8 * (e >> 2) + 4 * hh;
      f[e] += coef * (ex[e] * rse - (v == yv[i] ? 1.f : 0.f)) * Z[i][e];
    }
  }
#pragma unroll
  for (int e = 0; e < 16; ++e) {
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) f[e] += __shfl_xor(f[e], o, 64);
  }
  lsum = wave_reduce_sum(lsum);
  if (r == 0) {
#pragma unroll
    for (int e = 0; e < 16; ++e) tred[w * VP + (e & 3) + 8 * (e >> 2) + 4 * hh] = f[e];
  }
  if (lane == 0) lred[w] = lsum;
  __syncthreads();
  if (tid < VP) {
    float a = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) a += tred[k * VP + tid];
    tt[tid] = a;
  }
  if (tid == 0) {
    float a = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) a += lred[k];
    loss_part[l] = a * inv_bl;
  }
  __syncthreads();
  // (4) per tile: dZ = P (G - T), dz rows, dh^T = Wo^T dZ^T, 256-B row stores
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    m[e] = tt[(e & 3) + 8 * (e >> 2) + 4 * hh];
    f[e] = 0.f;
  }
  unsigned char* myot = ot + w * PT * OP_OTS;
#pragma unroll
  for (int i = 0; i < TPW; ++i) {
    const int t = w + 8 * i;
    if (t >= NT) break;
    const int s = t * 32 + r;
    const float coef = wg[i] * inv_bl;
    const int yl = yv[i] - 4 * hh;                     // the label among this lane's tokens
    float d[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const float ge = coef * __expf(Z[i][e] - lse[i]);                    // coef exp(P) / se
      const float G = (e & 3) + 8 * (e >> 2) == yl ? ge - coef : ge;
      d[e] = Z[i][e] * (G - m[e]);
      f[e] += d[e];
    }
    if (s < B) {
      bf16_t* dst = dz + ((size_t)s * L + l) * VP + 4 * hh;
#pragma unroll
      for (int g = 0; g < 4; ++g) *reinterpret_cast<uint2*>(dst + 8 * g) = packq4(d + 4 * g);
    }
    // A = Wo^T (row = channel, K = v): lane K slots 8 hh + j <-> v = 16 kk + 4 hh + j (j < 4),
    // 16 kk + 8 + 4 hh + j - 4 (j >= 4), the tokens of this lane's d[8 kk + j]
    const bf16x8 fa[2] = {pack8(d), pack8(d + 8)};
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      f32x16_t acc = zero16();
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const int rlo = kk * 16 + 4 * hh + q, col = ct * 32 + tc;
        const bf16x8 fb = cat_tr(lds_tr(wos, swz256e(rlo, col)), lds_tr(wos, swz256e(rlo + 8, col)));
        acc = mfma32(fb, fa[kk], acc);
      }
      // D[channel ct * 32 + (e & 3) + 8 (e >> 2) + 4 hh][sample r]: 4 consecutive channels per register quad
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float o4[4] = {acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
        *reinterpret_cast<uint2*>(myot + r * OP_OTS + 8 * hh + (ct * 4 + g) * 16) = packq4(o4);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int idx = lane + 64 * k;                 // 512 16-B chunks = 32 rows x 16
      const int rr = idx >> 4, c8 = idx & 15;
      const int sr = t * 32 + rr;
      if (sr < B)
        *reinterpret_cast<uint4*>(dh + ((size_t)sr * L + l) * CH + c8 * 8) =
            *reinterpret_cast<const uint4*>(myot + rr * OP_OTS + c8 * 16);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  // (5) dbo partial
#pragma unroll
  for (int e = 0; e < 16; ++e) {
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) f[e] += __shfl_xor(f[e], o, 64);
  }
  if (r == 0) {
#pragma unroll
    for (int e = 0; e < 16; ++e) dbr[w * VP + (e & 3) + 8 * (e >> 2) + 4 * hh] = f[e];
  }
  __syncthreads();
  if (tid < V) {
    float a = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) a += dbr[k * VP + tid];
    dbo_part[(size_t)l * V + tid] = a;
  }
}
}  // namespace

// Workspace sizes (floats) for pbx_local_head3_a/_b/_c: Z [B*L*32], part/tpart [ceil(B/16) * L * 32 * 2] each,
// MS/T [L * 32 * 2] each, loss_part / dbo_part [ntiles], [ntiles * V]; ntiles = ceil(B/16) ceil(L/32).
PBX_EXPORT int pbx_local_head3_tiles(int B, int L) { return ((B + SB - 1) / SB) * ((L + PT - 1) / PT); }

namespace {
constexpr int LDS1 = VP * 256 + VP * 4 + SB * PT * (VP + 1) * 4;
constexpr int LDS5 = 8 * PT * 256 + VP * 256 + PT * VP * 8 + PT * VP * 4 + VP * 4 + 8 * VP * 4;
void lhead3_attrs() {
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)lhead_logits_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LDS1);
    (void)hipFuncSetAttribute((const void*)lhead_grad_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LDS5);
    attr = true;
  }
}
}  // namespace

// The five passes in three stages, so that a data-parallel group can share the batch axis of the softmax
// (parallel/batch_softmax.py): stage A = passes 1-2 -- with raw = 1 the fold leaves (M, S) for the caller
// to merge over ranks into (M, 1/S) --, stage B = passes 3-4 (T, which the caller sums over ranks),
// stage C = pass 5.  Outputs: dh [B][L][128] bf16, dz [B*L][32] bf16 (for dWo = dz^T h, a GEMM the caller
// issues), dbo_part [ntiles][V], loss_part [ntiles] (each already divided by B L).
PBX_EXPORT int pbx_local_head3_a(const void* h, const float* wo, const float* bo, float* Z, float* part, float* MS,
                                 int raw, int B, int L, int V, hipStream_t st) {
  if (V > VP || V < 1 || B < 1 || L < 1) return (int)hipErrorInvalidValue;
  lhead3_attrs();
  const int nt = pbx_local_head3_tiles(B, L);
  const int nch = (B + SB - 1) / SB;
  hipLaunchKernelGGL(lhead_logits_kernel, dim3(nt), dim3(512), LDS1, st, (const bf16_t*)h, wo, bo, Z, (float2*)part,
                     B, L, V);
  hipLaunchKernelGGL(lhead_fold_kernel, dim3((L * VP + 63) / 64), dim3(256), 0, st, (const float2*)part, nch, L,
                     (float2*)MS, raw ? 2 : 0);
  return pbx_launch_status();
}

PBX_EXPORT int pbx_local_head3_b(const float* Z, const float* MS, const void* y, const float* wl, float* tpart,
                                 float* loss_part, float* T, int B, int L, int V, hipStream_t st) {
  if (V > VP || V < 1 || B < 1 || L < 1) return (int)hipErrorInvalidValue;
  const int nt = pbx_local_head3_tiles(B, L);
  const int nch = (B + SB - 1) / SB;
  const float inv_bl = 1.0f / ((float)B * (float)L);
  hipLaunchKernelGGL(lhead_ce_kernel, dim3(nt), dim3(512), 0, st, Z, (const float2*)MS, (const long long*)y, wl,
                     (float2*)tpart, loss_part, B, L, V, inv_bl);
  hipLaunchKernelGGL(lhead_fold_kernel, dim3((L * VP + 63) / 64), dim3(256), 0, st, (const float2*)tpart, nch, L,
                     (float2*)T, 1);
  return pbx_launch_status();
}

PBX_EXPORT int pbx_local_head3_c(const float* Z, const float* MS, const float* T, const void* y, const float* wl,
                                 const float* wo, const float* bo, void* dh, void* dz, float* dbo_part, int B, int L,
                                 int V, hipStream_t st) {
  if (V > VP || V < 1 || B < 1 || L < 1) return (int)hipErrorInvalidValue;
  lhead3_attrs();
  const int nt = pbx_local_head3_tiles(B, L);
  const float inv_bl = 1.0f / ((float)B * (float)L);
  hipLaunchKernelGGL(lhead_grad_kernel, dim3(nt), dim3(512), LDS5, st, Z, (const float2*)MS, (const float2*)T,
                     (const long long*)y, wl, wo, bo, (bf16_t*)dh, (bf16_t*)dz, dbo_part, B, L, V, inv_bl);
  return pbx_launch_status();
}

// Positions per workgroup of pbx_local_head_fused: 1 for B <= 2048 (0: unsupported, the caller takes the
// five-pass form).  Sizes its outputs: dbo_part [ceil(L / pp)][V], loss_part [ceil(L / pp)].
PBX_EXPORT int pbx_local_head_fused_pp(int B) { return B >= 1 && B <= 2048 ? 1 : 0; }

// One-launch head (B <= 2048): dbo_part [L][V], loss_part [L] (each already / (B L)).  The kernel is
// instantiated for 2, 4 and 8 row tiles per wave (B <= 512, 1024, 2048): fewer logits registers leave room
// for a second workgroup per CU at the smaller batches.
PBX_EXPORT int pbx_local_head_fused(const void* h, const float* wo, const float* bo, const void* y, const float* wl,
                                    void* dh, void* dz, float* dbo_part, float* loss_part, int B, int L, int V,
                                    hipStream_t st) {
  if (V > VP || V < 1 || pbx_local_head_fused_pp(B) == 0 || L < 1) return (int)hipErrorInvalidValue;
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)lhead_onepass_kernel<8>, hipFuncAttributeMaxDynamicSharedMemorySize, OP_LDS);
    (void)hipFuncSetAttribute((const void*)lhead_onepass_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, OP_LDS);
    (void)hipFuncSetAttribute((const void*)lhead_onepass_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, OP_LDS);
    attr = true;
  }
  const float inv_bl = 1.0f / ((float)B * (float)L);
  auto k = B <= 512 ? lhead_onepass_kernel<2> : B <= 1024 ? lhead_onepass_kernel<4> : lhead_onepass_kernel<8>;
  hipLaunchKernelGGL(k, dim3(L), dim3(512), OP_LDS, st, (const bf16_t*)h, wo, bo, (const long long*)y, wl,
                     (bf16_t*)dh, (bf16_t*)dz, dbo_part, loss_part, B, L, V, inv_bl);
  return pbx_launch_status();
}


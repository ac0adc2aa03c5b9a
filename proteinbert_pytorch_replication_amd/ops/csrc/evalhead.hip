// Held-out evaluation heads: the pretraining heads' losses and prediction counts without any gradient.
//
// The training heads (csrc/lhead.hip, csrc/phead.hip, EPI_GO in csrc/gemm.hip) produce the loss together
// with dh / dz, a [B*L, 32] and a [B, A] gradient an evaluation throws away.  Here every head writes only
// per-tile partials -- one fp32 loss partial and four unsigned counts for the local head, one loss partial
// and 2 x 256 histogram bins for the GO head (EPI_GO_EVAL, csrc/gemm.hip) -- and one fold launch per batch
// adds them, in a fixed order, into a persistent device accumulator (fp64 loss sums, int64 counts and
// histograms), so an evaluation over many batches needs no host sync and cannot overflow.
//
// Counts per tile, over the rows with weight w > 0:
//   [0] rows                      [1] hits (argmax_v P == y) among them
//   [2] rows with x != y          [3] hits among those       (x: input tokens, y: targets -> the corrupted positions)
// argmax over v < V, lowest index on ties.
//
// Reference semantics (softmax over the BATCH axis, ProteinBERT/modules.py:277-284): the (M, 1/S)
// statistics of every (l, v) come from stage A of the training head (pbx_local_head3_a: logits Z and the
// folded statistics); lhead_eval_kernel is one more pass over the same 16-sample x 32-position row tiles:
//   P[v] = exp(Z - M) / S ;  CE term w (log sum_v exp(P[v]) - P[y]) / (B L)  (lhead_ce_kernel's formula).
// Paper semantics (softmax over the vocabulary): phead_eval_kernel is phead_kernel without its gradient half.
#include "mfma.h"

using namespace pbx;
typedef unsigned short bf16_t;

namespace {
constexpr int CH = 128;
constexpr int SB = 16;     // samples per tile (reference semantics)
constexpr int PT = 32;     // positions per tile
constexpr int VP = 32;     // padded vocabulary
constexpr int NCNT = 4;    // counts per tile
constexpr int NBIN = 256;  // GO-score histogram bins per class

// (value, index) argmax merge keeping the lowest index on ties
__device__ __forceinline__ void amax_merge(float& bv, int& bi, float ov, int oi) {
  if (ov > bv || (ov == bv && oi < bi)) {
    bv = ov;
    bi = oi;
  }
}

__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (unsigned)__shfl_xor((int)v, o, 64);
  return v;
}

// the four counts of one row, as a packed per-lane increment (only one lane of a row counts it)
__device__ __forceinline__ void count_row(unsigned (&c)[NCNT], bool counted, bool hit, bool corrupted) {
  c[0] += counted ? 1u : 0u;
  c[1] += counted && hit ? 1u : 0u;
  c[2] += counted && corrupted ? 1u : 0u;
  c[3] += counted && corrupted && hit ? 1u : 0u;
}

// ---- reference semantics: one pass over Z with the folded (M, 1/S).  Tiles and the lane -> (row, tokens)
// map are lhead_ce_kernel's: wave w owns samples 2w, 2w + 1 of the tile, lane (r, hh) row p0 + r and the 16
// tokens v = 8 hh + j (j < 8), 16 + 8 hh + j.
__global__ void __launch_bounds__(512) lhead_eval_kernel(const float* __restrict__ Z, const float2* __restrict__ MS,
                                                         const long long* __restrict__ y,
                                                         const long long* __restrict__ x,
                                                         const float* __restrict__ wl, float* __restrict__ loss_part,
                                                         unsigned* __restrict__ cnt_part, int B, int L, int V,
                                                         float inv_bl) {
  __shared__ float2 ms[PT * VP];
  __shared__ float red[8];
  __shared__ unsigned cred[8][NCNT];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r = lane & 31, hh = lane >> 5;
  const int TP = (L + PT - 1) / PT;
  const int chunk = blockIdx.x / TP;
  const int b0 = chunk * SB, p0 = (blockIdx.x - chunk * TP) * PT;
  for (int i = tid; i < PT * VP; i += 512) {
    const int pp = min(p0 + i / VP, L - 1);
    ms[i] = MS[(size_t)pp * VP + (i % VP)];
  }
  __syncthreads();
  float lsum = 0.f;
  unsigned cnt[NCNT] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int si = 0; si < 2; ++si) {
    const int b = b0 + 2 * w + si, pos = p0 + r;
    const bool ok = b < B && pos < L;
    const size_t row = (size_t)min(b, B - 1) * L + min(pos, L - 1);     // clamped: loads in bounds
    const int yv = (int)y[row];
    const int xv = (int)x[row];
    const float wgt = ok ? wl[row] : 0.f;
    float zv[16];
    {
      const float4* zp0 = reinterpret_cast<const float4*>(Z + row * VP + 8 * hh);
      const float4* zp1 = reinterpret_cast<const float4*>(Z + row * VP + 16 + 8 * hh);
      const float4 a = zp0[0], bq = zp0[1], c = zp1[0], d = zp1[1];
      const float tmp[16] = {a.x, a.y, a.z, a.w, bq.x, bq.y, bq.z, bq.w, c.x, c.y, c.z, c.w, d.x, d.y, d.z, d.w};
#pragma unroll
      for (int j = 0; j < 16; ++j) zv[j] = tmp[j];
    }
    float se = 0.f, py = 0.f, bv = -1.f;
    int bi = VP;
#pragma unroll
    for (int j = 0; j < 16; ++j) {                  // v ascending in j: a strict > keeps the lowest index
      const int v = (j < 8 ? 0 : 16) + 8 * hh + (j & 7);
      const float2 s = ms[r * VP + v];
      const bool inv = v < V;
      const float P = inv ? __expf(zv[j] - s.x) * s.y : 0.f;
      se += inv ? __expf(P) : 0.f;
      py += v == yv ? P : 0.f;
      if (inv && P > bv) {
        bv = P;
        bi = v;
      }
    }
    se += __shfl_xor(se, 32, 64);
    amax_merge(bv, bi, __shfl_xor(bv, 32, 64), __shfl_xor(bi, 32, 64));
    // this lane's share of w (log se - P[y]), as lhead_ce_kernel sums it
    lsum += ok ? wgt * ((hh == 0 ? __logf(se) : 0.f) - py) : 0.f;
    count_row(cnt, ok && hh == 0 && wgt > 0.f, bi == yv, xv != yv);
  }
  lsum = wave_reduce_sum(lsum);
#pragma unroll
  for (int k = 0; k < NCNT; ++k) cnt[k] = wave_sum_u32(cnt[k]);
  if (lane == 0) {
    red[w] = lsum;
#pragma unroll
    for (int k = 0; k < NCNT; ++k) cred[w][k] = cnt[k];
  }
  __syncthreads();
  if (tid == 0) {
    float s = 0.f;
#pragma unroll
    for (int ww = 0; ww < 8; ++ww) s += red[ww];
    loss_part[blockIdx.x] = s * inv_bl;
  }
  if (tid < NCNT) {
    unsigned s = 0u;
#pragma unroll
    for (int ww = 0; ww < 8; ++ww) s += cred[ww][tid];
    cnt_part[(size_t)blockIdx.x * NCNT + tid] = s;
  }
}

// ---- paper semantics: phead_kernel's forward half.  One wave per 32-row tile (grid-stride), Z^T = Wo h^T on
// MFMA: a lane holds the 16 logits v = (e & 3) + 8 (e >> 2) + 4 hh of ONE row.  The argmax is taken on the
// logits (the row softmax is monotone in them).
__global__ void __launch_bounds__(256) phead_eval_kernel(const bf16_t* __restrict__ h, const float* __restrict__ wo,
                                                         const float* __restrict__ bo, const long long* __restrict__ y,
                                                         const long long* __restrict__ x, const float* __restrict__ wl,
                                                         float* __restrict__ loss_part, unsigned* __restrict__ cnt_part,
                                                         long R, int V, float inv_bl) {
  __shared__ __attribute__((aligned(16))) unsigned char wos[VP * 256];   // Wo bf16 [32][128] swz256
  __shared__ float bo_s[VP];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r = lane & 31, hh = lane >> 5;
  for (int idx = tid; idx < VP * 16; idx += 256) {
    const int v = idx >> 4, c8 = idx & 15;
    float e[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (v < V) {
      const float4 a = *reinterpret_cast<const float4*>(wo + v * CH + c8 * 8);
      const float4 b = *reinterpret_cast<const float4*>(wo + v * CH + c8 * 8 + 4);
      e[0] = a.x; e[1] = a.y; e[2] = a.z; e[3] = a.w; e[4] = b.x; e[5] = b.y; e[6] = b.z; e[7] = b.w;
    }
    *reinterpret_cast<uint4*>(wos + swz256(v, c8)) = packq8(e);
  }
  if (tid < VP) bo_s[tid] = tid < V ? bo[tid] : 0.f;
  __syncthreads();
  bf16x8 wf[8];                                     // A = Wo rows (v = r), k = channels
#pragma unroll
  for (int kk = 0; kk < 8; ++kk) wf[kk] = lds_frag(wos, swz256(r, kk * 2 + hh));
  float bov[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) bov[e] = bo_s[(e & 3) + 8 * (e >> 2) + 4 * hh];
  float lsum = 0.f;
  unsigned cnt[NCNT] = {0u, 0u, 0u, 0u};
  const long ntile = (R + 31) / 32;
  for (long t = (long)blockIdx.x * 4 + w; t < ntile; t += (long)gridDim.x * 4) {
    const long row = t * 32 + r;
    const bool ok = row < R;
    const long rc = ok ? row : R - 1;
    const bf16_t* src = h + rc * CH + 8 * hh;
    bf16x8 hf[8];
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) hf[kk] = *reinterpret_cast<const bf16x8*>(src + kk * 16);
    const int yv = ok ? (int)y[rc] : -1;
    const int xv = ok ? (int)x[rc] : -1;
    const float wraw = ok ? wl[rc] : 0.f;
    const float wgt = wraw * inv_bl;
    f32x16_t z = zero16();
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) z = mfma32(wf[kk], hf[kk], z);   // z[e]: v = (e&3) + 8(e>>2) + 4 hh, row r
    float m = -3.0e38f;
    int bi = VP;
#pragma unroll
    for (int e = 0; e < 16; ++e) {                  // v ascending in e: a strict > keeps the lowest index
      const int v = (e & 3) + 8 * (e >> 2) + 4 * hh;
      z[e] = v < V ? z[e] + bov[e] : -3.0e38f;
      if (v < V && z[e] > m) {
        m = z[e];
        bi = v;
      }
    }
    amax_merge(m, bi, __shfl_xor(m, 32, 64), __shfl_xor(bi, 32, 64));
    float se = 0.f, zy = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int v = (e & 3) + 8 * (e >> 2) + 4 * hh;
      se += v < V ? __expf(z[e] - m) : 0.f;
      zy += v == yv ? z[e] : 0.f;
    }
    se += __shfl_xor(se, 32, 64);
    zy += __shfl_xor(zy, 32, 64);
    if (hh == 0) lsum += ok ? wgt * (m + __logf(se) - zy) : 0.f;
    count_row(cnt, ok && hh == 0 && wraw > 0.f, bi == yv, xv != yv);
  }
  const long wid = (long)blockIdx.x * 4 + w;
  lsum = wave_reduce_sum(lsum);
#pragma unroll
  for (int k = 0; k < NCNT; ++k) cnt[k] = wave_sum_u32(cnt[k]);
  if (lane == 0) {
    loss_part[wid] = lsum;
#pragma unroll
    for (int k = 0; k < NCNT; ++k) cnt_part[wid * NCNT + k] = cnt[k];
  }
}

// ---- fold: partials of one batch -> the persistent accumulator.  Block 0: both heads' loss partials (summed
// in fp64: every thread a strided slice, then a fixed tree) and the local head's counts; blocks 1 ..: 16 bins
// of the 2 x 256 GO histogram each (64-B runs of a partial row), the workgroup rows split over 16 thread
// groups with four loads in flight per thread (a thread walking its rows one dependent load at a time made
// the fold as long as the heads themselves at 1120 GO tiles).
//   acc_loss [2] fp64: sum of the batches' local / GO loss
//   acc_cnt  [8 + 512] int64: batches, sequences, the four counts, 2 reserved, hist(y = 1) [256], hist(y = 0) [256]
__global__ void __launch_bounds__(256) eval_fold_kernel(const float* __restrict__ lloss, const unsigned* __restrict__ lcnt,
                                                        int nl, const float* __restrict__ gloss,
                                                        const unsigned* __restrict__ ghist, int ng,
                                                        double* __restrict__ acc_loss, long long* __restrict__ acc_cnt,
                                                        int B) {
  __shared__ double dred[2][256];
  __shared__ unsigned long long ured[16][64];       // block 0: [4 counts][256] (the same 8 KB); else [16 groups][16 bins]
  const int tid = threadIdx.x;
  if (blockIdx.x == 0) {
    double a = 0.0, g = 0.0;
    unsigned long long c[NCNT] = {0ull, 0ull, 0ull, 0ull};
    for (int i = tid; i < nl; i += 256) {
      a += (double)lloss[i];
#pragma unroll
      for (int k = 0; k < NCNT; ++k) c[k] += lcnt[(size_t)i * NCNT + k];
    }
    for (int i = tid; i < ng; i += 256) g += (double)gloss[i];
    dred[0][tid] = a;
    dred[1][tid] = g;
    unsigned long long (*cred)[256] = reinterpret_cast<unsigned long long (*)[256]>(&ured[0][0]);
#pragma unroll
    for (int k = 0; k < NCNT; ++k) cred[k][tid] = c[k];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (tid < s) {
        dred[0][tid] += dred[0][tid + s];
        dred[1][tid] += dred[1][tid + s];
#pragma unroll
        for (int k = 0; k < NCNT; ++k) cred[k][tid] += cred[k][tid + s];
      }
      __syncthreads();
    }
    if (tid < 2) acc_loss[tid] += dred[tid][0];
    if (tid == 2) acc_cnt[0] += 1;
    if (tid == 3) acc_cnt[1] += B;
    if (tid >= 4 && tid < 4 + NCNT) acc_cnt[2 + (tid - 4)] += (long long)cred[tid - 4][0];
    return;
  }
  const int bl = tid & 15, rg = tid >> 4;
  const int bin = (blockIdx.x - 1) * 16 + bl;                              // bin < 2 * NBIN (32 blocks)
  const unsigned* src = ghist + bin;
  unsigned long long s = 0ull;
  int i = rg;
  for (; i + 48 < ng; i += 64) {
    const unsigned a = src[(size_t)i * (2 * NBIN)], b = src[(size_t)(i + 16) * (2 * NBIN)],
                   c = src[(size_t)(i + 32) * (2 * NBIN)], d = src[(size_t)(i + 48) * (2 * NBIN)];
    s += (unsigned long long)a + b + c + d;
  }
  for (; i < ng; i += 16) s += src[(size_t)i * (2 * NBIN)];
  ured[rg][bl] = s;
  __syncthreads();
  if (rg == 0) {
    unsigned long long t = 0ull;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += ured[k][bl];
    acc_cnt[8 + bin] += (long long)t;
  }
}
}  // namespace

// Reference-semantics local head, evaluation pass: Z [B*L][32] fp32 and MS [L][32] (M, 1/S) from
// pbx_local_head3_a (merged over ranks by the caller when the batch softmax is shared), y / x [B*L] int64
// targets / input tokens, wl [B*L] weights -> loss_part [tiles] (each already divided by B L), cnt_part
// [tiles][4]; tiles = pbx_local_head3_tiles(B, L).
PBX_EXPORT int pbx_local_head_eval(const float* Z, const float* MS, const void* y, const void* x, const float* wl,
                                   float* loss_part, unsigned* cnt_part, int B, int L, int V, hipStream_t st) {
  if (V > VP || V < 1 || B < 1 || L < 1) return (int)hipErrorInvalidValue;
  const int nt = ((B + SB - 1) / SB) * ((L + PT - 1) / PT);
  const float inv_bl = 1.0f / ((float)B * (float)L);
  hipLaunchKernelGGL(lhead_eval_kernel, dim3(nt), dim3(512), 0, st, Z, (const float2*)MS, (const long long*)y,
                     (const long long*)x, wl, loss_part, cnt_part, B, L, V, inv_bl);
  return pbx_launch_status();
}

// Per-wave partial rows written by pbx_phead_eval (loss_part [n], cnt_part [n][4]).
PBX_EXPORT int pbx_phead_eval_parts(long R) {
  long ntile = (R + 31) / 32;
  long wg = (ntile + 3) / 4;
  if (wg > 1024) wg = 1024;
  return (int)(wg * 4);
}

// Paper-semantics local head, evaluation: h [R][128] bf16, wo [V][128] fp32, bo [V], y / x [R] int64, wl [R]
// fp32 -> loss_part [parts] (each already times inv_bl = 1 / (B L)), cnt_part [parts][4].
PBX_EXPORT int pbx_phead_eval(const void* h, const float* wo, const float* bo, const void* y, const void* x,
                              const float* wl, float* loss_part, unsigned* cnt_part, long R, int V, float inv_bl,
                              hipStream_t st) {
  if (V < 1 || V > VP || R < 1) return (int)hipErrorInvalidValue;
  const int parts = pbx_phead_eval_parts(R);
  hipLaunchKernelGGL(phead_eval_kernel, dim3(parts / 4), dim3(256), 0, st, (const bf16_t*)h, wo, bo,
                     (const long long*)y, (const long long*)x, wl, loss_part, cnt_part, R, V, inv_bl);
  return pbx_launch_status();
}

// One batch's partials into the accumulator: lloss [nl], lcnt [nl][4] (either local head), gloss [ng], ghist
// [ng][512] (pbx_go_head_eval), acc_loss [2] fp64, acc_cnt [520] int64 (layout above), B sequences.
PBX_EXPORT int pbx_eval_fold(const float* lloss, const unsigned* lcnt, int nl, const float* gloss,
                             const unsigned* ghist, int ng, double* acc_loss, long long* acc_cnt, int B,
                             hipStream_t st) {
  if (nl < 0 || ng < 0 || B < 0) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(eval_fold_kernel, dim3(1 + 2 * NBIN / 16), dim3(256), 0, st, lloss, lcnt, nl, gloss, ghist, ng,
                     acc_loss, acc_cnt, B);
  return pbx_launch_status();
}

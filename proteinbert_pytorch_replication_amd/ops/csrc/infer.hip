// Inference heads (ops/infer_heads.py): what a prediction needs from the encoder outputs, without loss,
// gradient or targets.  Every output is written with plain stores by exactly one thread: no atomics,
// results bitwise repeatable.
//
//   pbx_row_topk          the k largest entries of every row of an fp32 matrix (the GO probabilities of
//                         pbx_go_head_probs, EPI_GO_PROB in csrc/gemm.hip), descending, equal values in
//                         ascending index order: torch.sort(descending=True, stable=True)[:k].
//   pbx_local_probs_ref   reference-semantics local head (softmax over the BATCH axis): one more pass over
//                         the Z [B*L][32] / (M, 1/S) of pbx_local_head3_a, like lhead_eval_kernel
//                         (csrc/evalhead.hip) and with its P = exp(Z - M) (1/S) expression.
//   pbx_phead_probs       paper-semantics local head (softmax over the vocabulary): phead_eval_kernel's
//                         MFMA forward half.
//   pbx_masked_mean_pool  mean of h [B][L][128] over the positions whose token is not <pad>.
//
// Both local heads write P [rows][V] fp32 (dense, optional), tok [rows] int32 = the lowest index of the
// maximum of the STORED row of P (two logits can round to one fp32 probability: the argmax is taken on
// what is stored, so the outputs agree with each other) and pmax [rows] = P[tok].
#include "mfma.h"

#include <math.h>

using namespace pbx;
typedef unsigned short bf16_t;

namespace {
constexpr int CH = 128;
constexpr int SB = 16;     // samples per tile (reference semantics)
constexpr int PT = 32;     // positions per tile
constexpr int VP = 32;     // padded vocabulary

// (value, index) argmax merge keeping the lowest index on ties
__device__ __forceinline__ void amax_merge(float& bv, int& bi, float ov, int oi) {
  if (ov > bv || (ov == bv && oi < bi)) {
    bv = ov;
    bi = oi;
  }
}

// ---- top-k.  One wave per row, the row resident in registers: lane holds columns j * 64 + lane, j < NPL
// (coalesced 256-B loads, the row read once).  k rounds: every lane's local maximum (ascending j and a
// strict >: its lowest column on ties), a 6-step (value, column) butterfly keeping the lowest column on
// ties, then the owner lane retires the winner (-inf) inside the next round's scan.  Every array index is
// a compile-time constant: the row never leaves the registers.  Lane t keeps round t's result; one
// coalesced store per output at the end.
template <int NPL>
__global__ void __launch_bounds__(64) row_topk_kernel(const float* __restrict__ P, long ld, int A, int k,
                                                      float* __restrict__ val, int* __restrict__ idx) {
  const int lane = threadIdx.x;
  const float* row = P + (size_t)blockIdx.x * ld;
  const float NEG = -INFINITY;
  float v[NPL];
#pragma unroll
  for (int j = 0; j < NPL; ++j) {
    const int c = j * 64 + lane;
    v[j] = c < A ? row[c] : NEG;
  }
  float rv = 0.f;
  int ri = 0;
  int retire = -1;                                   // this lane's j to retire in the coming scan
  for (int t = 0; t < k; ++t) {
    float bv = NEG;
    int bj = 0;
#pragma unroll
    for (int j = 0; j < NPL; ++j) {
      v[j] = j == retire ? NEG : v[j];
      if (v[j] > bv) {
        bv = v[j];
        bj = j;
      }
    }
    int bc = bj * 64 + lane;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amax_merge(bv, bc, __shfl_xor(bv, o, 64), __shfl_xor(bc, o, 64));
    retire = (bc & 63) == lane ? bc >> 6 : -1;
    if (lane == t) {
      rv = bv;
      ri = bc;
    }
  }
  if (lane < k) {
    val[(size_t)blockIdx.x * k + lane] = rv;
    idx[(size_t)blockIdx.x * k + lane] = ri;
  }
}

// ---- reference semantics: lhead_eval_kernel's tiles and lane -> (row, tokens) map: wave w owns samples
// 2w, 2w + 1 of the tile, lane (r, hh) row p0 + r and the 16 tokens v = 8 hh + j (j < 8), 16 + 8 hh + j.
__global__ void __launch_bounds__(512) lprobs_ref_kernel(const float* __restrict__ Z, const float2* __restrict__ MS,
                                                         float* __restrict__ P, int* __restrict__ tok,
                                                         float* __restrict__ pmax, int store_p, int B, int L,
                                                         int V) {
  __shared__ float2 ms[PT * VP];
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
#pragma unroll
  for (int si = 0; si < 2; ++si) {
    const int b = b0 + 2 * w + si, pos = p0 + r;
    const bool ok = b < B && pos < L;
    const size_t row = (size_t)min(b, B - 1) * L + min(pos, L - 1);     // clamped: loads in bounds
    float zv[16];
    {
      const float4* zp0 = reinterpret_cast<const float4*>(Z + row * VP + 8 * hh);
      const float4* zp1 = reinterpret_cast<const float4*>(Z + row * VP + 16 + 8 * hh);
      const float4 a = zp0[0], bq = zp0[1], c = zp1[0], d = zp1[1];
      const float tmp[16] = {a.x, a.y, a.z, a.w, bq.x, bq.y, bq.z, bq.w, c.x, c.y, c.z, c.w, d.x, d.y, d.z, d.w};
#pragma unroll
      for (int j = 0; j < 16; ++j) zv[j] = tmp[j];
    }
    float bv = -1.f;
    int bi = VP;
    float* prow = P + row * V;
#pragma unroll
    for (int j = 0; j < 16; ++j) {                  // v ascending in j: a strict > keeps the lowest index
      const int v = (j < 8 ? 0 : 16) + 8 * hh + (j & 7);
      const float2 s = ms[r * VP + v];
      const bool inv = v < V;
      const float p = inv ? __expf(zv[j] - s.x) * s.y : 0.f;
      if (inv && p > bv) {
        bv = p;
        bi = v;
      }
      if (store_p && ok && inv) prow[v] = p;
    }
    amax_merge(bv, bi, __shfl_xor(bv, 32, 64), __shfl_xor(bi, 32, 64));
    if (ok && hh == 0) {
      tok[row] = bi;
      pmax[row] = bv;
    }
  }
}

// ---- paper semantics: phead_eval_kernel's forward half.  One wave per 32-row tile (grid-stride), Z^T = Wo h^T
// on MFMA: a lane holds the 16 logits v = (e & 3) + 8 (e >> 2) + 4 hh of ONE row; P = exp(z - max) (1 / sum).
__global__ void __launch_bounds__(256) phead_probs_kernel(const bf16_t* __restrict__ h, const float* __restrict__ wo,
                                                          const float* __restrict__ bo, float* __restrict__ P,
                                                          int* __restrict__ tok, float* __restrict__ pmax,
                                                          int store_p, long R, int V) {
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
  const long ntile = (R + 31) / 32;
  for (long t = (long)blockIdx.x * 4 + w; t < ntile; t += (long)gridDim.x * 4) {
    const long row = t * 32 + r;
    const bool ok = row < R;
    const long rc = ok ? row : R - 1;
    const bf16_t* src = h + rc * CH + 8 * hh;
    bf16x8 hf[8];
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) hf[kk] = *reinterpret_cast<const bf16x8*>(src + kk * 16);
    f32x16_t z = zero16();
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) z = mfma32(wf[kk], hf[kk], z);   // z[e]: v = (e&3) + 8(e>>2) + 4 hh, row r
    float m = -3.0e38f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int v = (e & 3) + 8 * (e >> 2) + 4 * hh;
      z[e] = v < V ? z[e] + bov[e] : -3.0e38f;
      m = fmaxf(m, z[e]);
    }
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    float se = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int v = (e & 3) + 8 * (e >> 2) + 4 * hh;
      z[e] = v < V ? __expf(z[e] - m) : 0.f;
      se += z[e];
    }
    se += __shfl_xor(se, 32, 64);
    const float inv = 1.0f / se;
    float bv = -1.f;
    int bi = VP;
    float* prow = P + rc * V;
#pragma unroll
    for (int e = 0; e < 16; ++e) {                  // v ascending in e: a strict > keeps the lowest index
      const int v = (e & 3) + 8 * (e >> 2) + 4 * hh;
      const float p = z[e] * inv;
      if (v < V && p > bv) {
        bv = p;
        bi = v;
      }
      if (store_p && ok && v < V) prow[v] = p;
    }
    amax_merge(bv, bi, __shfl_xor(bv, 32, 64), __shfl_xor(bi, 32, 64));
    if (ok && hh == 0) {
      tok[rc] = bi;
      pmax[rc] = bv;
    }
  }
}

// ---- masked mean pool.  One workgroup per sequence; thread (pg, c8) = (tid >> 4, tid & 15) owns channels
// 8 c8 .. + 7 (one 16-B load per position) and the positions pg, pg + 16, ..., summed in that order in fp32;
// the 16 position groups are then added in ascending pg by the threads of group 0.  A <pad> position is
// not loaded at all.
__global__ void __launch_bounds__(256) masked_mean_pool_kernel(const bf16_t* __restrict__ h,
                                                               const long long* __restrict__ tokens,
                                                               float* __restrict__ out, int L) {
  __shared__ float part[16][CH + 4];
  __shared__ int cpart[16];
  const int tid = threadIdx.x, c8 = tid & 15, pg = tid >> 4;
  const size_t b = blockIdx.x;
  const bf16_t* hb = h + b * (size_t)L * CH + 8 * c8;
  const long long* tb = tokens + b * (size_t)L;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int cnt = 0;
#pragma unroll 4
  for (int p = pg; p < L; p += 16) {
    if (tb[p] != 0) {
      const uint4 q = *reinterpret_cast<const uint4*>(hb + (size_t)p * CH);
      float f[8];
      unpack8(q, f);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += f[e];
      ++cnt;
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) part[pg][8 * c8 + e] = acc[e];
  if (c8 == 0) cpart[pg] = cnt;
  __syncthreads();
  if (tid < CH) {
    float s = 0.f;
    int n = 0;
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      s += part[g][tid];
      n += cpart[g];
    }
    out[b * CH + tid] = n > 0 ? s / (float)n : 0.f;
  }
}
}  // namespace

// P [B][ld] fp32 (A columns used; finite values), 1 <= k <= min(64, A), A <= 16384 (the limits that
// ops/infer_heads.topk_supported publishes) -> val [B][k] fp32, idx [B][k] int32: the k largest of each row,
// descending, equal values by ascending column.
PBX_EXPORT int pbx_row_topk(const float* P, long ld, int B, int A, int k, float* val, int* idx, hipStream_t st) {
  if (B < 1 || A < 1 || A > 256 * 64 || k < 1 || k > 64 || k > A || ld < A) return (int)hipErrorInvalidValue;
  auto kern = A <= 2 * 64 ? row_topk_kernel<2> : A <= 16 * 64 ? row_topk_kernel<16> : A <= 64 * 64 ? row_topk_kernel<64>
              : A <= 144 * 64 ? row_topk_kernel<144> : row_topk_kernel<256>;
  hipLaunchKernelGGL(kern, dim3(B), dim3(64), 0, st, P, ld, A, k, val, idx);
  return pbx_launch_status();
}

// Reference-semantics local head, prediction pass: Z [B*L][32] fp32 and MS [L][32] (M, 1/S) from
// pbx_local_head3_a -> P [B*L][V] fp32 (skipped when store_p == 0; P may then be null), tok [B*L] int32,
// pmax [B*L] fp32.
PBX_EXPORT int pbx_local_probs_ref(const float* Z, const float* MS, float* P, int* tok, float* pmax, int store_p,
                                   int B, int L, int V, hipStream_t st) {
  if (V > VP || V < 1 || B < 1 || L < 1 || (store_p && P == nullptr)) return (int)hipErrorInvalidValue;
  const int nt = ((B + SB - 1) / SB) * ((L + PT - 1) / PT);
  hipLaunchKernelGGL(lprobs_ref_kernel, dim3(nt), dim3(512), 0, st, Z, (const float2*)MS, P, tok, pmax, store_p, B, L,
                     V);
  return pbx_launch_status();
}

// Paper-semantics local head, prediction: h [R][128] bf16, wo [V][128] fp32, bo [V] -> P [R][V] fp32 (skipped
// when store_p == 0), tok [R] int32, pmax [R] fp32.
PBX_EXPORT int pbx_phead_probs(const void* h, const float* wo, const float* bo, float* P, int* tok, float* pmax,
                               int store_p, long R, int V, hipStream_t st) {
  if (V < 1 || V > VP || R < 1 || (store_p && P == nullptr)) return (int)hipErrorInvalidValue;
  long wg = ((R + 31) / 32 + 3) / 4;
  if (wg > 1024) wg = 1024;
  hipLaunchKernelGGL(phead_probs_kernel, dim3((unsigned)wg), dim3(256), 0, st, (const bf16_t*)h, wo, bo, P, tok, pmax,
                     store_p, R, V);
  return pbx_launch_status();
}

// h [B][L][128] bf16, tokens [B][L] int64 -> out [B][128] fp32: the mean of h over the positions with
// token != 0 (<pad>), zeros for a sequence without one.
PBX_EXPORT int pbx_masked_mean_pool(const void* h, const void* tokens, float* out, int B, int L, hipStream_t st) {
  if (B < 1 || L < 1) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(masked_mean_pool_kernel, dim3(B), dim3(256), 0, st, (const bf16_t*)h, (const long long*)tokens,
                     out, L);
  return pbx_launch_status();
}

// Sequence and variant scores from the local head's logits (ops/infer_heads.local_scores): the same in both
// semantics, a function of one row's h, its token and the head weights alone.
//
//   pbx_lhead_scores    z[v] = h . bf16(Wo[v]) + bo[v] exactly as pbx_phead_probs forms it (csrc/infer.hip: one
//                       wave per 32-row tile, Wo as MFMA A-fragments from LDS once per workgroup, 16 of the 32
//                       padded logits of ONE row per lane, the row's two half-lanes combined by
//                       __shfl_xor(.., 32)).  With x the row's token and the row LIVE when UNK_ID <= x < V:
//                         llr[v]  = z[v] - z[x]                      (optional store; column x is +0.0)
//                         logp    = (z[x] - m) - log(sum_v exp(z[v] - m)),  m = max_v z[v]
//                         entropy = log(sum_v e_v) - (sum_v e_v d_v) / (sum_v e_v),  d_v = z[v] - m, e_v = exp(d_v)
//                       (both entropy terms are >= 0: no cancellation).  A row that is not live gets zeros; its
//                       token indexes nothing.  The logits never leave the registers.
//   pbx_seq_score_fold  per sequence: n_live and pll = the sum of the stored logp over the live positions, in
//                       fp64: thread t adds positions t, t + 64, ... in ascending order, lane 0 adds the 64
//                       partials in ascending t, one rounding to fp32.  The order depends on L alone.
//
// Every output is written with a plain store by exactly one thread: no atomics, results bitwise repeatable
// and independent of the batch size, the grid and the row's place in its tile.
#include "mfma.h"

#include <math.h>

using namespace pbx;
typedef unsigned short bf16_t;

namespace {
constexpr int CH = 128;
constexpr int VP = 32;        // padded vocabulary
constexpr int UNK_ID = 3;     // data/vocab.py: <pad>, <sos>, <eos> lie below it and are not scored
constexpr int MAX_WG = 1024;  // grid cap of pbx_lhead_scores (4 tiles per workgroup and trip)

__device__ __forceinline__ bool live_token(long long x, int V) { return x >= UNK_ID && x < V; }

__global__ void __launch_bounds__(256) lhead_scores_kernel(const bf16_t* __restrict__ h, const float* __restrict__ wo,
                                                           const float* __restrict__ bo,
                                                           const long long* __restrict__ tokens,
                                                           float* __restrict__ llr, float* __restrict__ logp,
                                                           float* __restrict__ entropy, int store_llr, long R, int V) {
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
    const long rc = ok ? row : R - 1;                // clamped: loads in bounds, nothing stored
    const bf16_t* src = h + rc * CH + 8 * hh;
    bf16x8 hf[8];
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) hf[kk] = *reinterpret_cast<const bf16x8*>(src + kk * 16);
    const long long x64 = tokens[rc];
    const bool live = live_token(x64, V);
    const int x = live ? (int)x64 : -1;              // -1 matches no column
    f32x16_t z = zero16();
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) z = mfma32(wf[kk], hf[kk], z);   // z[e]: v = (e&3) + 8(e>>2) + 4 hh, row r
    float m = -3.0e38f, zx = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {                  // the predicated walk: z[x] from the half that holds it
      const int v = (e & 3) + 8 * (e >> 2) + 4 * hh;
      z[e] += bov[e];
      m = v < V ? fmaxf(m, z[e]) : m;
      zx = v == x ? z[e] : zx;
    }
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    const float zo = __shfl_xor(zx, 32, 64);
    zx = ((x >> 2) & 1) == hh ? zx : zo;            // a select, not a sum: -0.0 stays -0.0
    float se = 0.f, sd = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int v = (e & 3) + 8 * (e >> 2) + 4 * hh;
      const float d = z[e] - m;
      const float ev = v < V ? __expf(d) : 0.f;
      se += ev;
      sd = v < V ? fmaf(ev, d, sd) : sd;
    }
    se += __shfl_xor(se, 32, 64);
    sd += __shfl_xor(sd, 32, 64);
    const float lse = logf(se);
    if (store_llr && ok) {
      float* lrow = llr + row * V;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int v = (e & 3) + 8 * (e >> 2) + 4 * hh;
        if (v < V) lrow[v] = (live && v != x) ? z[e] - zx : 0.f;
      }
    }
    if (ok && hh == 0) {
      logp[row] = live ? (zx - m) - lse : 0.f;
      entropy[row] = live ? lse - sd / se : 0.f;
    }
  }
}

// One wave per sequence (the shape of masked_mean_pool_kernel: a fixed position stride per thread, then the
// partials in ascending order).  A position that is not live is not loaded.
__global__ void __launch_bounds__(64) seq_score_fold_kernel(const float* __restrict__ logp,
                                                            const long long* __restrict__ tokens,
                                                            float* __restrict__ pll, int* __restrict__ n_live, int L,
                                                            int V) {
  __shared__ double part[64];
  __shared__ int cpart[64];
  const int tid = threadIdx.x;
  const size_t b = blockIdx.x;
  const float* lb = logp + b * (size_t)L;
  const long long* tb = tokens + b * (size_t)L;
  double acc = 0.0;
  int cnt = 0;
  for (int p = tid; p < L; p += 64) {
    if (live_token(tb[p], V)) {
      acc += (double)lb[p];
      ++cnt;
    }
  }
  part[tid] = acc;
  cpart[tid] = cnt;
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    int n = 0;
    for (int g = 0; g < 64; ++g) {
      s += part[g];
      n += cpart[g];
    }
    pll[b] = (float)s;
    n_live[b] = n;
  }
}
}  // namespace

// h [R][128] bf16, wo [V][128] fp32, bo [V], tokens [R] int64 -> llr [R][V] fp32 (skipped when store_llr == 0;
// llr may then be null), logp [R], entropy [R] fp32.  1 <= V <= 32.
PBX_EXPORT int pbx_lhead_scores(const void* h, const float* wo, const float* bo, const void* tokens, float* llr,
                                float* logp, float* entropy, int store_llr, long R, int V, hipStream_t st) {
  if (V < 1 || V > VP || R < 1 || h == nullptr || wo == nullptr || bo == nullptr || tokens == nullptr ||
      logp == nullptr || entropy == nullptr || (store_llr && llr == nullptr))
    return (int)hipErrorInvalidValue;
  long wg = ((R + 31) / 32 + 3) / 4;
  if (wg > MAX_WG) wg = MAX_WG;
  hipLaunchKernelGGL(lhead_scores_kernel, dim3((unsigned)wg), dim3(256), 0, st, (const bf16_t*)h, wo, bo,
                     (const long long*)tokens, llr, logp, entropy, store_llr, R, V);
  return pbx_launch_status();
}

// logp [B][L] fp32 (of pbx_lhead_scores), tokens [B][L] int64 -> pll [B] fp32, n_live [B] int32; a sequence
// without a live position gets pll = 0, n_live = 0.
PBX_EXPORT int pbx_seq_score_fold(const float* logp, const void* tokens, float* pll, int* n_live, int B, int L, int V,
                                  hipStream_t st) {
  if (V < 1 || V > VP || B < 1 || L < 1 || logp == nullptr || tokens == nullptr || pll == nullptr ||
      n_live == nullptr)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(seq_score_fold_kernel, dim3(B), dim3(64), 0, st, logp, (const long long*)tokens, pll, n_live, L,
                     V);
  return pbx_launch_status();
}

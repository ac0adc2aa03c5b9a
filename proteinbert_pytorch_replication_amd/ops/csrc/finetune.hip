// Per-residue fine-tuning head weight gradient (BASELINE cfg 5: frozen encoder + token classifier).
//
//   dW[k][c] = sum_rows g[row][k] h[row][c]        h: [M, 128] bf16 (encoder output), g: [M, K] fp32
//
// M = B * L = 262,144 rows and K = 8 classes: a hipBLASLt GEMM with the 262,144-long reduction axis
// ran 230 us (bf16) / 410 us (fp32) per step, a third of the whole fine-tune step; this kernel streams
// h once (64 MB) with fp32 accumulation.  Workgroup = 16 row lanes x 16 channel chunks of 8; each
// thread keeps its [KT][8] partial in registers over the workgroup's rows, the 4 row lanes of a wave
// are summed by shuffles and the 4 waves through LDS; every workgroup writes one partial row of a
// [P][K * 128] slab that pbx_colsum_add folds (deterministic, no atomics).
#include "mfma.h"

using namespace pbx;
typedef unsigned short bf16_t;

namespace {
constexpr int CH = 128;

template <int KT>
__global__ void __launch_bounds__(256) token_head_wgrad_kernel(const bf16_t* __restrict__ h,
                                                               const float* __restrict__ g, float* __restrict__ slab,
                                                               long M, int K) {
  __shared__ float red[4][KT * CH];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int rl = tid >> 4, cc = tid & 15;
  float acc[KT][8];
#pragma unroll
  for (int k = 0; k < KT; ++k)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[k][e] = 0.f;
  for (long row = (long)blockIdx.x * 16 + rl; row < M; row += (long)gridDim.x * 16) {
    const uint4 q = *reinterpret_cast<const uint4*>(h + row * CH + cc * 8);
    float hv[8];
    unpack8(q, hv);
    float gv[KT];
#pragma unroll
    for (int k = 0; k < KT; ++k) gv[k] = k < K ? g[row * K + k] : 0.f;
#pragma unroll
    for (int k = 0; k < KT; ++k)
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[k][e] = fmaf(gv[k], hv[e], acc[k][e]);
  }
  // lanes l, l^16, l^32, l^48 of a wave share the channel chunk
#pragma unroll
  for (int k = 0; k < KT; ++k)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      acc[k][e] += __shfl_xor(acc[k][e], 16, 64);
      acc[k][e] += __shfl_xor(acc[k][e], 32, 64);
    }
  if (lane < 16) {
#pragma unroll
    for (int k = 0; k < KT; ++k)
#pragma unroll
      for (int e = 0; e < 8; ++e) red[w][k * CH + cc * 8 + e] = acc[k][e];
  }
  __syncthreads();
  float* dst = slab + (size_t)blockIdx.x * K * CH;
  for (int i = tid; i < K * CH; i += 256) dst[i] = red[0][i] + red[1][i] + red[2][i] + red[3][i];
}
// Token-head logits (reference finetuning head, nn.Linear(128, K) on every residue):
//   out[m][k] = b[k] + sum_c h[m][c] W[k][c]
// A workgroup stages 256 rows (64 KiB) into LDS with coalesced 16-B loads (swz256 rows, so the
// row-per-thread reads below are conflict-free), then each thread owns one row: fp32 FMAs over the
// exact bf16 inputs and the fp32 weights (broadcast from LDS).  The library path needed two bf16 GEMMs
// on a hi / lo weight split for the same accuracy.
template <int K>
__global__ void __launch_bounds__(256) token_head_fwd_kernel(const bf16_t* __restrict__ h, const float* __restrict__ W,
                                                             const float* __restrict__ b, float* __restrict__ out,
                                                             long M) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // 256 rows x 256 B
  __shared__ float ws[K * CH];
  for (int i = threadIdx.x; i < K * CH; i += 256) ws[i] = W[i];
  const long m0 = (long)blockIdx.x * 256;
  const int n = (int)min((long)256, M - m0);
  stage_chunks(
      256 * 16,
      [&](int idx) {
        return (idx >> 4) < n ? *reinterpret_cast<const uint4*>(h + (m0 + (idx >> 4)) * CH + (idx & 15) * 8)
                              : make_uint4(0u, 0u, 0u, 0u);
      },
      [&](int idx, uint4 v) { *reinterpret_cast<uint4*>(smem + swz256(idx >> 4, idx & 15)) = v; });
  __syncthreads();
  const int row = threadIdx.x;
  if (row >= n) return;
  float acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = b[k];
#pragma unroll 4
  for (int c = 0; c < 16; ++c) {
    float v[8];
    unpack8(*reinterpret_cast<const uint4*>(smem + swz256(row, c)), v);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float* wr = ws + k * CH + c * 8;
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[k] = fmaf(v[e], wr[e], acc[k]);
    }
  }
  float* o = out + (m0 + row) * K;
#pragma unroll
  for (int k = 0; k < K; ++k) o[k] = acc[k];
}

template <int K>
int token_head_fwd_launch(const void* h, const float* W, const float* b, float* out, long M, hipStream_t st) {
  static bool attr = false;                  // 64 KiB dynamic + the static weight copy exceed the default
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)token_head_fwd_kernel<K>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              256 * 256);
    attr = true;
  }
  hipLaunchKernelGGL(token_head_fwd_kernel<K>, dim3((unsigned)((M + 255) / 256)), dim3(256), 256 * 256, st,
                     (const bf16_t*)h, W, b, out, M);
  return pbx_launch_status();
}

// ---- heads over every block's hidden state (hidden="all"): nb <= 8 sources of [M][128] bf16 ----
// The source addresses travel in the kernel's by-value argument block (no device-side table, no copy).
constexpr int MAXSRC = 8;
struct MultiSrc {
  const bf16_t* p[MAXSRC];
};

//   out[m][k] = b[k] + sum_i sum_c h_i[m][c] W[k][i * 128 + c]  (+ gterm[m / L][k])
// token_head_fwd_kernel's scheme with the block walk inside the workgroup: a thread keeps its row's K
// accumulators in registers across the nb blocks (blocks ascending, channels ascending inside a block: for
// nb = 1 and no gterm the FMA sequence is token_head_fwd_kernel's), gterm is added last and out is written
// once.  Every block's 256 rows and [K][128] weight slice pass through one 64 KiB + K * 512 B LDS image, so two
// workgroups stay resident per CU; the next block's rows are fetched into registers (16 x 16 B per thread)
// before the FMAs over the current image and stored after them, which hides the fetch behind the compute.
// (A second LDS image instead of the registers leaves one workgroup per CU and ran 1.8x slower at the cfg-5
// shape; no prefetch at all 1.1x slower: profiles/r15/finetune_hidden_heads.txt.)  Rows >= M are neither read
// nor written.
template <int K>
__global__ void __launch_bounds__(256) token_head_multi_fwd_kernel(const MultiSrc src, const int nb,
                                                                   const float* __restrict__ W,
                                                                   const float* __restrict__ b,
                                                                   const float* __restrict__ gterm,
                                                                   float* __restrict__ out, long M, int L) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // 256 rows x 256 B
  __shared__ float ws[K * CH];
  const long m0 = (long)blockIdx.x * 256;
  const int n = (int)min((long)256, M - m0);
  const int row = threadIdx.x;
  const int ldw = nb * CH;
  float acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = b[k];
  uint4 pre[16];                             // chunk idx = tid + 256 j of block i: row idx >> 4, 16-B chunk idx & 15
  auto fetch = [&](int i) {
    const bf16_t* __restrict__ h = src.p[i];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int idx = threadIdx.x + j * 256;
      pre[j] = (idx >> 4) < n ? *reinterpret_cast<const uint4*>(h + (m0 + (idx >> 4)) * CH + (idx & 15) * 8)
                              : make_uint4(0u, 0u, 0u, 0u);
    }
  };
  auto stage = [&](int i) {                  // the fetched rows (swz256: conflict-free row reads) + W[:, block i]
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int idx = threadIdx.x + j * 256;
      *reinterpret_cast<uint4*>(smem + swz256(idx >> 4, idx & 15)) = pre[j];
    }
    for (int j = threadIdx.x; j < K * CH; j += 256) ws[j] = W[(j >> 7) * ldw + i * CH + (j & (CH - 1))];
  };
  fetch(0);
  stage(0);
  __syncthreads();
  for (int i = 0; i < nb; ++i) {
    if (i + 1 < nb) fetch(i + 1);
    if (row < n) {
#pragma unroll 4
      for (int c = 0; c < 16; ++c) {
        float v[8];
        unpack8(*reinterpret_cast<const uint4*>(smem + swz256(row, c)), v);
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const float* wr = ws + k * CH + c * 8;
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[k] = fmaf(v[e], wr[e], acc[k]);
        }
      }
    }
    if (i + 1 < nb) {
      __syncthreads();                       // every thread is done with block i's image
      stage(i + 1);
      __syncthreads();
    }
  }
  if (row >= n) return;
  if (gterm != nullptr) {
    const float* gt = gterm + ((m0 + row) / L) * K;
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] += gt[k];
  }
  float* o = out + (m0 + row) * K;
#pragma unroll
  for (int k = 0; k < K; ++k) o[k] = acc[k];
}

template <int K>
int token_head_multi_fwd_launch(const MultiSrc& src, int nb, const float* W, const float* b, const float* gterm,
                                float* out, long M, int L, hipStream_t st) {
  static bool attr = false;                  // 64 KiB dynamic + the static weight slice exceed the default
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)token_head_multi_fwd_kernel<K>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, 256 * 256);
    attr = true;
  }
  hipLaunchKernelGGL(token_head_multi_fwd_kernel<K>, dim3((unsigned)((M + 255) / 256)), dim3(256), 256 * 256, st,
                     src, nb, W, b, gterm, out, M, L);
  return pbx_launch_status();
}

//   dW[k][i * 128 + c] = sum_m g[m][k] h_i[m][c]
// One row of the concatenated features is nb * 16 chunks of 8 channels: thread = (row lane rl, block i,
// chunk cc) with RL = 256 / (nb * 16) row lanes (threads past RL * nb * 16 idle), so a g row is fetched once
// per workgroup for all nb blocks and each thread keeps the [KT][8] partial of its (i, cc) in registers over
// the workgroup's rows (4 rows in flight per thread).  The row lanes are then summed in order through LDS and
// the workgroup writes partial row blockIdx.x of the [P][K][nb * 128] slab (fixed order, no atomics).
template <int KT>
__global__ void __launch_bounds__(256) token_head_multi_wgrad_kernel(const MultiSrc src, const int nb,
                                                                     const float* __restrict__ g,
                                                                     float* __restrict__ slab, long M, int K) {
  __shared__ __attribute__((aligned(16))) float red[256 * 8];
  const int tid = threadIdx.x;
  const int tpr = nb * 16, RL = 256 / tpr;
  const int rl = tid / tpr, rem = tid - rl * tpr;
  const int i = rem >> 4, cc = rem & 15;
  const bool active = rl < RL;
  constexpr int U = KT <= 8 ? 4 : 2;         // rows in flight per thread (KT = 16 holds 128 accumulators)
  float acc[KT][8];
#pragma unroll
  for (int k = 0; k < KT; ++k)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[k][e] = 0.f;
  if (active) {
    const bf16_t* __restrict__ h = src.p[i] + cc * 8;
    const long S = (long)gridDim.x * RL;
    long row = (long)blockIdx.x * RL + rl;
    for (; row + (U - 1) * S < M; row += U * S) {
      uint4 q[U];
      float gv[U][KT];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        q[u] = *reinterpret_cast<const uint4*>(h + (row + u * S) * CH);
#pragma unroll
        for (int k = 0; k < KT; ++k) gv[u][k] = k < K ? g[(row + u * S) * K + k] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        float hv[8];
        unpack8(q[u], hv);
#pragma unroll
        for (int k = 0; k < KT; ++k)
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[k][e] = fmaf(gv[u][k], hv[e], acc[k][e]);
      }
    }
    for (; row < M; row += S) {
      float hv[8];
      unpack8(*reinterpret_cast<const uint4*>(h + row * CH), hv);
#pragma unroll
      for (int k = 0; k < KT; ++k) {
        const float gk = k < K ? g[row * K + k] : 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[k][e] = fmaf(gk, hv[e], acc[k][e]);
      }
    }
  }
  float* dst = slab + (size_t)blockIdx.x * K * nb * CH + rem * 8;
#pragma unroll
  for (int k = 0; k < KT; ++k) {
    if (k < K) {                             // uniform: the barriers below are reached by every thread
      __syncthreads();                       // the previous class's partials have been summed
      if (active) {
        *reinterpret_cast<float4*>(red + tid * 8) = make_float4(acc[k][0], acc[k][1], acc[k][2], acc[k][3]);
        *reinterpret_cast<float4*>(red + tid * 8 + 4) = make_float4(acc[k][4], acc[k][5], acc[k][6], acc[k][7]);
      }
      __syncthreads();
      if (tid < tpr) {
        float s[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) s[e] = red[tid * 8 + e];
        for (int r = 1; r < RL; ++r)
#pragma unroll
          for (int e = 0; e < 8; ++e) s[e] += red[(r * tpr + tid) * 8 + e];
        float* d = dst + (size_t)k * nb * CH;
        *reinterpret_cast<float4*>(d) = make_float4(s[0], s[1], s[2], s[3]);
        *reinterpret_cast<float4*>(d + 4) = make_float4(s[4], s[5], s[6], s[7]);
      }
    }
  }
}

// ---- prediction with a trained per-residue head: calls and probabilities instead of logits ----
//   z[m][k] = b[k] + sum_i sum_c h_i[m][c] W[k][i * 128 + c]  (+ gterm[m / L][k])
//   P[m][k] = exp(z[m][k] - max_k z) / sum_k exp(z[m][k] - max_k z)
//   label[m] = the lowest k whose computed P[m][k] is maximal, pmax[m] = that P
// Staging, prefetch and FMA order are token_head_multi_fwd_kernel's, statement for statement (one 64 KiB LDS
// image, the next block in registers, blocks ascending, gterm last), so the logits a thread holds after the
// block walk are bit for bit the ones that kernel stores; they never leave the registers.  The epilogue is
// K values per thread: row maximum, __expf, the sum in ascending k, one division per class, and a strict >
// scan in ascending k (pbx_phead_probs' rule: the call is exact on the probabilities as computed).  A row whose
// token is below min_token holds no residue (<pad>, <sos>, <eos>): label -1, pmax 0 and a zero probability row;
// its FMAs are skipped (a wave of pads costs only the staging).  Rows >= M are neither read nor written.
template <int K>
__global__ void __launch_bounds__(256) token_head_calls_kernel(const MultiSrc src, const int nb,
                                                               const float* __restrict__ W,
                                                               const float* __restrict__ b,
                                                               const float* __restrict__ gterm,
                                                               const long long* __restrict__ tokens,
                                                               const int min_token, float* __restrict__ probs,
                                                               int* __restrict__ labels, float* __restrict__ pmax,
                                                               long M, int L) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // 256 rows x 256 B
  __shared__ float ws[K * CH];
  const long m0 = (long)blockIdx.x * 256;
  const int n = (int)min((long)256, M - m0);
  const int row = threadIdx.x;
  const int ldw = nb * CH;
  // the token is needed only after the block walk: issued first, its latency is behind the first staging
  const bool live = row < n && (tokens == nullptr || tokens[m0 + row] >= (long long)min_token);
  float acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = b[k];
  uint4 pre[16];                             // chunk idx = tid + 256 j of block i: row idx >> 4, 16-B chunk idx & 15
  auto fetch = [&](int i) {
    const bf16_t* __restrict__ h = src.p[i];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int idx = threadIdx.x + j * 256;
      pre[j] = (idx >> 4) < n ? *reinterpret_cast<const uint4*>(h + (m0 + (idx >> 4)) * CH + (idx & 15) * 8)
                              : make_uint4(0u, 0u, 0u, 0u);
    }
  };
  auto stage = [&](int i) {                  // the fetched rows (swz256: conflict-free row reads) + W[:, block i]
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int idx = threadIdx.x + j * 256;
      *reinterpret_cast<uint4*>(smem + swz256(idx >> 4, idx & 15)) = pre[j];
    }
    for (int j = threadIdx.x; j < K * CH; j += 256) ws[j] = W[(j >> 7) * ldw + i * CH + (j & (CH - 1))];
  };
  fetch(0);
  stage(0);
  __syncthreads();
  for (int i = 0; i < nb; ++i) {
    if (i + 1 < nb) fetch(i + 1);
    if (live) {
#pragma unroll 4
      for (int c = 0; c < 16; ++c) {
        float v[8];
        unpack8(*reinterpret_cast<const uint4*>(smem + swz256(row, c)), v);
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const float* wr = ws + k * CH + c * 8;
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[k] = fmaf(v[e], wr[e], acc[k]);
        }
      }
    }
    if (i + 1 < nb) {
      __syncthreads();                       // every thread is done with block i's image
      stage(i + 1);
      __syncthreads();
    }
  }
  if (row >= n) return;
  float* pr = probs != nullptr ? probs + (m0 + row) * K : nullptr;
  if (!live) {
    labels[m0 + row] = -1;
    pmax[m0 + row] = 0.f;
    if (pr != nullptr) {
#pragma unroll
      for (int k = 0; k < K; ++k) pr[k] = 0.f;
    }
    return;
  }
  if (gterm != nullptr) {
    const float* gt = gterm + ((m0 + row) / L) * K;
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] += gt[k];
  }
  float mx = acc[0];
#pragma unroll
  for (int k = 1; k < K; ++k) mx = fmaxf(mx, acc[k]);
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    acc[k] = __expf(acc[k] - mx);
    s += acc[k];
  }
  float bv = -1.f;
  int bi = 0;
#pragma unroll
  for (int k = 0; k < K; ++k) {              // k ascending: a strict > keeps the lowest index
    acc[k] = acc[k] / s;
    if (acc[k] > bv) {
      bv = acc[k];
      bi = k;
    }
  }
  labels[m0 + row] = bi;
  pmax[m0 + row] = bv;
  if (pr != nullptr) {
#pragma unroll
    for (int k = 0; k < K; ++k) pr[k] = acc[k];
  }
}

template <int K>
int token_head_calls_launch(const MultiSrc& src, int nb, const float* W, const float* b, const float* gterm,
                            const long long* tokens, int min_token, float* probs, int* labels, float* pmax, long M,
                            int L, hipStream_t st) {
  static bool attr = false;                  // 64 KiB dynamic + the static weight slice exceed the default
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)token_head_calls_kernel<K>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              256 * 256);
    attr = true;
  }
  hipLaunchKernelGGL(token_head_calls_kernel<K>, dim3((unsigned)((M + 255) / 256)), dim3(256), 256 * 256, st, src,
                     nb, W, b, gterm, tokens, min_token, probs, labels, pmax, M, L);
  return pbx_launch_status();
}

// ---- evaluation of a trained per-residue head: cross-entropy and a K x K confusion table instead of calls ----
//   z[m][k] as above;  call[m] = token_head_calls_kernel's label;  ce[m] = log sum_k exp(z - max z) - (z_y - max z)
// Staging, prefetch and FMA order are token_head_calls_kernel's, statement for statement, so the logits a thread
// holds are bit for bit that kernel's (and token_head_multi_fwd_kernel's) and its call is that kernel's label.
// Row classes by the label y[m]: y < 0 is ignored (the -100 of the loaders; its FMAs are skipped), y >= K is a
// bad label (counted in slot K*K + 1, otherwise ignored), every other row is live: one LDS integer atomic on
// cm[y * K + call], one on the live-row count (slot K*K).  Workgroup w owns rows 256 w .. 256 w + 255 and writes
// loss_part[w] (lane-ordered wave reduction, then waves 0..3 in order: no float atomics, bitwise repeatable) and
// cnt_part[w][K*K + 2].  The LDS image grows by the table alone (<= 1032 B): two workgroups still fit a CU.
// Rows >= M are neither read nor counted; the logits are never written.
template <int K>
__global__ void __launch_bounds__(256) token_head_eval_kernel(const MultiSrc src, const int nb,
                                                              const float* __restrict__ W,
                                                              const float* __restrict__ b,
                                                              const float* __restrict__ gterm,
                                                              const long long* __restrict__ y,
                                                              float* __restrict__ loss_part,
                                                              unsigned* __restrict__ cnt_part, long M, int L) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // 256 rows x 256 B
  __shared__ float ws[K * CH];
  constexpr int NC = K * K + 2;
  __shared__ unsigned cm[NC];
  __shared__ float wsum[4];
  const long m0 = (long)blockIdx.x * 256;
  const int n = (int)min((long)256, M - m0);
  const int row = threadIdx.x;
  const int ldw = nb * CH;
  // the label is needed only after the block walk: issued first, its latency is behind the first staging
  const long long yv = row < n ? y[m0 + row] : -1ll;
  const bool live = yv >= 0 && yv < (long long)K;
  for (int j = threadIdx.x; j < NC; j += 256) cm[j] = 0u;     // visible after the first staging barrier
  float acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = b[k];
  uint4 pre[16];                             // chunk idx = tid + 256 j of block i: row idx >> 4, 16-B chunk idx & 15
  auto fetch = [&](int i) {
    const bf16_t* __restrict__ h = src.p[i];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int idx = threadIdx.x + j * 256;
      pre[j] = (idx >> 4) < n ? *reinterpret_cast<const uint4*>(h + (m0 + (idx >> 4)) * CH + (idx & 15) * 8)
                              : make_uint4(0u, 0u, 0u, 0u);
    }
  };
  auto stage = [&](int i) {                  // the fetched rows (swz256: conflict-free row reads) + W[:, block i]
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int idx = threadIdx.x + j * 256;
      *reinterpret_cast<uint4*>(smem + swz256(idx >> 4, idx & 15)) = pre[j];
    }
    for (int j = threadIdx.x; j < K * CH; j += 256) ws[j] = W[(j >> 7) * ldw + i * CH + (j & (CH - 1))];
  };
  fetch(0);
  stage(0);
  __syncthreads();
  for (int i = 0; i < nb; ++i) {
    if (i + 1 < nb) fetch(i + 1);
    if (live) {
#pragma unroll 4
      for (int c = 0; c < 16; ++c) {
        float v[8];
        unpack8(*reinterpret_cast<const uint4*>(smem + swz256(row, c)), v);
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const float* wr = ws + k * CH + c * 8;
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[k] = fmaf(v[e], wr[e], acc[k]);
        }
      }
    }
    if (i + 1 < nb) {
      __syncthreads();                       // every thread is done with block i's image
      stage(i + 1);
      __syncthreads();
    }
  }
  float ce = 0.f;                            // no early return: every thread reaches the barriers below
  if (live) {
    if (gterm != nullptr) {
      const float* gt = gterm + ((m0 + row) / L) * K;
#pragma unroll
      for (int k = 0; k < K; ++k) acc[k] += gt[k];
    }
    const int yi = (int)yv;
    float mx = acc[0];
#pragma unroll
    for (int k = 1; k < K; ++k) mx = fmaxf(mx, acc[k]);
    float s = 0.f, zy = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      zy = k == yi ? acc[k] - mx : zy;
      acc[k] = __expf(acc[k] - mx);
      s += acc[k];
    }
    float bv = -1.f;
    int bi = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {            // k ascending: a strict > keeps the lowest index
      acc[k] = acc[k] / s;
      if (acc[k] > bv) {
        bv = acc[k];
        bi = k;
      }
    }
    ce = logf(s) - zy;
    atomicAdd(&cm[yi * K + bi], 1u);
    atomicAdd(&cm[K * K], 1u);
  } else if (yv >= (long long)K) {
    atomicAdd(&cm[K * K + 1], 1u);
  }
  ce = wave_reduce_sum(ce);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = ce;
  __syncthreads();                           // the table and the four wave sums are complete
  if (threadIdx.x == 0) loss_part[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
  unsigned* cp = cnt_part + (size_t)blockIdx.x * NC;
  for (int j = threadIdx.x; j < NC; j += 256) cp[j] = cm[j];
}

template <int K>
int token_head_eval_launch(const MultiSrc& src, int nb, const float* W, const float* b, const float* gterm,
                           const long long* y, float* loss_part, unsigned* cnt_part, long M, int L, hipStream_t st) {
  static bool attr = false;                  // 64 KiB dynamic + the static weight slice and table exceed the default
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)token_head_eval_kernel<K>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              256 * 256);
    attr = true;
  }
  hipLaunchKernelGGL(token_head_eval_kernel<K>, dim3((unsigned)((M + 255) / 256)), dim3(256), 256 * 256, st, src, nb,
                     W, b, gterm, y, loss_part, cnt_part, M, L);
  return pbx_launch_status();
}

// ---- fold: one batch's partials of token_head_eval_kernel -> the persistent accumulator (eval_fold_kernel's
// scheme, csrc/evalhead.hip).  Block (0, 0): the loss partials in fp64, ascending workgroup order at every level:
// thread t adds the contiguous run t * run .. (t + 1) * run - 1 (run = ceil(nwg / 256): one partial each up to 256
// workgroups; four loads in flight), threads 0..15 add the run sums 16 t .. 16 t + 15, thread 0 adds those 16
// (a single thread walking all 256 run sums made the fold a fifth of the head itself at 4096 workgroups); and the
// batch / sequence counters.  Blocks (1 .., s): 16 columns of the [nwg][K*K + 2] table each over the s-th of
// gridDim.y row ranges, the rows split over 16 thread groups with four loads in flight per thread; a block adds
// its column sums to the accumulator with 64-bit integer atomics (integers: exact in any order, so the result
// is the same on every launch).  No float atomics.
//   acc_loss [1] fp64;  acc_cnt [K*K + 4] int64: confusion [K][K] (true x predicted), live rows, bad labels,
//   batches, sequences
__global__ void __launch_bounds__(256) task_eval_fold_kernel(const float* __restrict__ loss_part,
                                                             const unsigned* __restrict__ cnt_part, int nwg, int nc,
                                                             int n_sequences, double* __restrict__ acc_loss,
                                                             long long* __restrict__ acc_cnt) {
  __shared__ double dred[256];
  __shared__ double dred2[16];
  __shared__ unsigned long long ured[16][16];
  const int tid = threadIdx.x;
  if (blockIdx.x == 0) {
    if (blockIdx.y != 0) return;
    const int run = (nwg + 255) / 256;
    const int i1 = min(nwg, (tid + 1) * run);
    int i = min(nwg, tid * run);
    double a = 0.0;
    for (; i + 3 < i1; i += 4) {
      const float v0 = loss_part[i], v1 = loss_part[i + 1], v2 = loss_part[i + 2], v3 = loss_part[i + 3];
      a += (double)v0;
      a += (double)v1;
      a += (double)v2;
      a += (double)v3;
    }
    for (; i < i1; ++i) a += (double)loss_part[i];
    dred[tid] = a;
    __syncthreads();
    if (tid < 16) {
      double s = dred[tid * 16];
#pragma unroll
      for (int t = 1; t < 16; ++t) s += dred[tid * 16 + t];
      dred2[tid] = s;
    }
    __syncthreads();
    if (tid == 0) {
      double s = dred2[0];
#pragma unroll
      for (int t = 1; t < 16; ++t) s += dred2[t];
      acc_loss[0] += s;
      acc_cnt[nc] += 1;
      acc_cnt[nc + 1] += n_sequences;
    }
    return;
  }
  const int cl = tid & 15, rg = tid >> 4;
  const int col = (blockIdx.x - 1) * 16 + cl;
  const int chunk = (nwg + (int)gridDim.y - 1) / (int)gridDim.y;
  const int r0 = (int)blockIdx.y * chunk, r1 = min(nwg, r0 + chunk);
  unsigned long long s = 0ull;
  if (col < nc) {
    const unsigned* src = cnt_part + col;
    int i = r0 + rg;
    for (; i + 48 < r1; i += 64) {
      const unsigned a = src[(size_t)i * nc], b = src[(size_t)(i + 16) * nc], c = src[(size_t)(i + 32) * nc],
                     d = src[(size_t)(i + 48) * nc];
      s += (unsigned long long)a + b + c + d;
    }
    for (; i < r1; i += 16) s += src[(size_t)i * nc];
  }
  ured[rg][cl] = s;
  __syncthreads();
  if (rg == 0 && col < nc) {
    unsigned long long t = 0ull;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += ured[k][cl];
    if (t != 0ull) atomicAdd(reinterpret_cast<unsigned long long*>(acc_cnt + col), t);
  }
}

// ---- training a per-residue head: the shaped cross-entropy and its logit gradient instead of the logits ----
//   z[m][k] as above;  p = softmax(z), lp = log p, w = cw (or ones), S = sum_k w_k, c = eps / K
//   loss_row = (1 - eps) w_y (-lp_y) + c sum_k w_k (-lp_k)          wrow = w_y
//   g[m][k]  = (1 - eps) w_y (p_k - [k == y]) + c (p_k S - w_k)
// which is F.cross_entropy(z, y, weight=cw, label_smoothing=eps) before its division by sum wrow: g is written
// unnormalised and the caller scales the reduced gradients by 1 / sum wrow (pbx_token_head_loss_fold's out[1]).
// Staging, prefetch and FMA order are token_head_eval_kernel's, statement for statement, so the logits a thread
// holds are bit for bit token_head_multi_fwd_kernel's and its call (p_k = exp / sum, strict > in ascending k) is
// token_head_calls_kernel's label.  Row classes as there: y < 0 ignored, y >= K a bad label (counted), both write
// a zero row of g (the weight-gradient kernels read every row < M) and skip their FMAs.  -lp_k is formed as
// log(sum) - (z_k - max), so K = 1 gives a loss of exactly +0 and a zero gradient.  Workgroup w writes
// part[w] = {sum loss_row, sum wrow} (lane-ordered wave reduction, then waves 0..3 in order) and cnt[w] =
// {live rows, hits, bad labels} (wave ballots: integers); no atomics at all.  The LDS image is the 64 KiB of rows,
// K * 512 B of weights and ten words.  Rows >= M are neither read nor written; the logits are never written.
template <int K>
__global__ void __launch_bounds__(256) token_head_loss_kernel(const MultiSrc src, const int nb,
                                                              const float* __restrict__ W,
                                                              const float* __restrict__ b,
                                                              const float* __restrict__ gterm,
                                                              const long long* __restrict__ y,
                                                              const float* __restrict__ cw, const float eps,
                                                              float* __restrict__ g, float* __restrict__ part,
                                                              unsigned* __restrict__ cnt, long M, int L) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // 256 rows x 256 B
  __shared__ float ws[K * CH];
  __shared__ float wsum[4][2];
  __shared__ unsigned wcnt[4][3];
  const long m0 = (long)blockIdx.x * 256;
  const int n = (int)min((long)256, M - m0);
  const int row = threadIdx.x;
  const int ldw = nb * CH;
  // the label is needed only after the block walk: issued first, its latency is behind the first staging
  const long long yv = row < n ? y[m0 + row] : -1ll;
  const bool live = yv >= 0 && yv < (long long)K;
  float acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = b[k];
  uint4 pre[16];                             // chunk idx = tid + 256 j of block i: row idx >> 4, 16-B chunk idx & 15
  auto fetch = [&](int i) {
    const bf16_t* __restrict__ h = src.p[i];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int idx = threadIdx.x + j * 256;
      pre[j] = (idx >> 4) < n ? *reinterpret_cast<const uint4*>(h + (m0 + (idx >> 4)) * CH + (idx & 15) * 8)
                              : make_uint4(0u, 0u, 0u, 0u);
    }
  };
  auto stage = [&](int i) {                  // the fetched rows (swz256: conflict-free row reads) + W[:, block i]
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int idx = threadIdx.x + j * 256;
      *reinterpret_cast<uint4*>(smem + swz256(idx >> 4, idx & 15)) = pre[j];
    }
    for (int j = threadIdx.x; j < K * CH; j += 256) ws[j] = W[(j >> 7) * ldw + i * CH + (j & (CH - 1))];
  };
  fetch(0);
  stage(0);
  __syncthreads();
  for (int i = 0; i < nb; ++i) {
    if (i + 1 < nb) fetch(i + 1);
    if (live) {
#pragma unroll 4
      for (int c = 0; c < 16; ++c) {
        float v[8];
        unpack8(*reinterpret_cast<const uint4*>(smem + swz256(row, c)), v);
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const float* wr = ws + k * CH + c * 8;
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[k] = fmaf(v[e], wr[e], acc[k]);
        }
      }
    }
    if (i + 1 < nb) {
      __syncthreads();                       // every thread is done with block i's image
      stage(i + 1);
      __syncthreads();
    }
  }
  float lrow = 0.f, wrow = 0.f;              // no early return: every thread reaches the barrier below
  bool hit = false;
  if (live) {
    if (gterm != nullptr) {
      const float* gt = gterm + ((m0 + row) / L) * K;
#pragma unroll
      for (int k = 0; k < K; ++k) acc[k] += gt[k];
    }
    const int yi = (int)yv;
    float wk[K];                             // uniform addresses: the class weights stay in scalar registers
    float S = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      wk[k] = cw != nullptr ? cw[k] : 1.f;
      S += wk[k];
    }
    float mx = acc[0];
#pragma unroll
    for (int k = 1; k < K; ++k) mx = fmaxf(mx, acc[k]);
    float d[K];                              // z_k - max
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      d[k] = acc[k] - mx;
      acc[k] = __expf(d[k]);
      s += acc[k];
    }
    const float lse = logf(s);
    float bv = -1.f, wy = 0.f, nly = 0.f, sm = 0.f;
    int bi = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {            // k ascending: a strict > keeps the lowest index
      acc[k] = acc[k] / s;
      if (acc[k] > bv) {
        bv = acc[k];
        bi = k;
      }
      const float nl = lse - d[k];           // -lp_k
      wy = k == yi ? wk[k] : wy;
      nly = k == yi ? nl : nly;
      sm = fmaf(wk[k], nl, sm);
    }
    const float a = (1.f - eps) * wy, c = eps / (float)K;
    lrow = a * nly + c * sm;
    wrow = wy;
    hit = bi == yi;
    float* gr = g + (m0 + row) * K;
#pragma unroll
    for (int k = 0; k < K; ++k) gr[k] = a * (acc[k] - (k == yi ? 1.f : 0.f)) + c * (acc[k] * S - wk[k]);
  } else if (row < n) {
    float* gr = g + (m0 + row) * K;
#pragma unroll
    for (int k = 0; k < K; ++k) gr[k] = 0.f;
  }
  const unsigned nlive = (unsigned)__popcll(__ballot(live));
  const unsigned nhit = (unsigned)__popcll(__ballot(hit));
  const unsigned nbad = (unsigned)__popcll(__ballot(yv >= (long long)K));
  lrow = wave_reduce_sum(lrow);
  wrow = wave_reduce_sum(wrow);
  if ((threadIdx.x & 63) == 0) {
    const int wv = threadIdx.x >> 6;
    wsum[wv][0] = lrow;
    wsum[wv][1] = wrow;
    wcnt[wv][0] = nlive;
    wcnt[wv][1] = nhit;
    wcnt[wv][2] = nbad;
  }
  __syncthreads();                           // the four waves' sums are complete
  if (threadIdx.x < 2)
    part[(size_t)blockIdx.x * 2 + threadIdx.x] =
        ((wsum[0][threadIdx.x] + wsum[1][threadIdx.x]) + wsum[2][threadIdx.x]) + wsum[3][threadIdx.x];
  else if (threadIdx.x >= 64 && threadIdx.x < 67) {
    const int j = threadIdx.x - 64;
    cnt[(size_t)blockIdx.x * 3 + j] = wcnt[0][j] + wcnt[1][j] + wcnt[2][j] + wcnt[3][j];
  }
}

template <int K>
int token_head_loss_launch(const MultiSrc& src, int nb, const float* W, const float* b, const float* gterm,
                           const long long* y, const float* cw, float eps, float* g, float* part, unsigned* cnt,
                           long M, int L, hipStream_t st) {
  static bool attr = false;                  // 64 KiB dynamic + the static weight slice exceed the default
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)token_head_loss_kernel<K>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              256 * 256);
    attr = true;
  }
  hipLaunchKernelGGL(token_head_loss_kernel<K>, dim3((unsigned)((M + 255) / 256)), dim3(256), 256 * 256, st, src, nb,
                     W, b, gterm, y, cw, eps, g, part, cnt, M, L);
  return pbx_launch_status();
}

// ---- fold: one batch's partials of token_head_loss_kernel -> the step's loss, gradient scale and accuracy.
// One block.  The two fp64 sums take task_eval_fold_kernel block (0, 0)'s order: thread t adds the contiguous run
// t * run .. (t + 1) * run - 1 (run = ceil(nwg / 256)) in ascending order, threads 0..15 add the run sums
// 16 t .. 16 t + 15, thread 0 adds those 16.  The three counters are integer sums (exact in any order).
//   out[0] = sum loss / sum w, out[1] = 1 / sum w (nan and 0 when sum w == 0: an all-ignored batch has a nan
//   loss and a zero gradient, as in torch), out[2] = hits / max(1, live);  acc_cnt [3] int64 += live, hits, bad
__global__ void __launch_bounds__(256) token_head_loss_fold_kernel(const float* __restrict__ part,
                                                                   const unsigned* __restrict__ cnt, int nwg,
                                                                   float* __restrict__ out,
                                                                   long long* __restrict__ acc_cnt) {
  __shared__ double dred[2][256];
  __shared__ double dred2[2][16];
  __shared__ unsigned long long ured[3][256];
  const int tid = threadIdx.x;
  const int run = (nwg + 255) / 256;
  const int i0 = min(nwg, tid * run), i1 = min(nwg, (tid + 1) * run);
  double a = 0.0, w = 0.0;
  unsigned long long c0 = 0ull, c1 = 0ull, c2 = 0ull;
  int i = i0;
  for (; i + 3 < i1; i += 4) {               // four partial rows' loads in flight, added in ascending order
    float p[8];
    unsigned c[12];
#pragma unroll
    for (int u = 0; u < 8; ++u) p[u] = part[2 * (size_t)i + u];
#pragma unroll
    for (int u = 0; u < 12; ++u) c[u] = cnt[3 * (size_t)i + u];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      a += (double)p[2 * u];
      w += (double)p[2 * u + 1];
      c0 += c[3 * u];
      c1 += c[3 * u + 1];
      c2 += c[3 * u + 2];
    }
  }
  for (; i < i1; ++i) {
    a += (double)part[2 * (size_t)i];
    w += (double)part[2 * (size_t)i + 1];
    c0 += cnt[3 * (size_t)i];
    c1 += cnt[3 * (size_t)i + 1];
    c2 += cnt[3 * (size_t)i + 2];
  }
  dred[0][tid] = a;
  dred[1][tid] = w;
  ured[0][tid] = c0;
  ured[1][tid] = c1;
  ured[2][tid] = c2;
  __syncthreads();
  if (tid < 32) {
    const int q = tid >> 4, t = tid & 15;
    double s = dred[q][t * 16];
#pragma unroll
    for (int j = 1; j < 16; ++j) s += dred[q][t * 16 + j];
    dred2[q][t] = s;
  } else if (tid >= 64 && tid < 67) {
    unsigned long long s = 0ull;
    for (int j = 0; j < 256; ++j) s += ured[tid - 64][j];
    ured[tid - 64][0] = s;                   // slot 0 is read by this thread alone before the barrier below
  }
  __syncthreads();
  if (tid == 0) {
    double sl = dred2[0][0], sw = dred2[1][0];
#pragma unroll
    for (int t = 1; t < 16; ++t) {
      sl += dred2[0][t];
      sw += dred2[1][t];
    }
    const unsigned long long live = ured[0][0], hits = ured[1][0], bad = ured[2][0];
    out[0] = sw == 0.0 ? __builtin_nanf("") : (float)(sl / sw);
    out[1] = sw == 0.0 ? 0.f : (float)(1.0 / sw);
    out[2] = (float)((double)hits / (double)(live > 0ull ? live : 1ull));
    acc_cnt[0] += (long long)live;
    acc_cnt[1] += (long long)hits;
    acc_cnt[2] += (long long)bad;
  }
}

bool multi_src(const void* const* srcs, int nb, MultiSrc& ms) {
  if (srcs == nullptr || nb < 1 || nb > MAXSRC) return false;
  for (int i = 0; i < MAXSRC; ++i) {
    ms.p[i] = (const bf16_t*)srcs[i < nb ? i : 0];
    if ((reinterpret_cast<uintptr_t>(ms.p[i]) & 15) != 0 || ms.p[i] == nullptr) return false;   // 16-B row loads
  }
  return true;
}
}  // namespace

// out [M][K] fp32 = b + sum_i h_i [M][128] bf16 . W[:, i*128:(i+1)*128]^T (W: [K][nb*128] fp32) + gterm[m / L]
// srcs: HOST array of the nb (<= 8) device addresses; gterm ([ceil(M / L)][K] fp32) may be null; K <= 16
PBX_EXPORT int pbx_token_head_multi_fwd(const void* const* srcs, int nb, const float* W, const float* b,
                                        const float* gterm, float* out, long M, int K, int L, hipStream_t st) {
  MultiSrc ms;
  if (M < 1 || L < 1 || !multi_src(srcs, nb, ms)) return (int)hipErrorInvalidValue;
  switch (K) {
    case 1: return token_head_multi_fwd_launch<1>(ms, nb, W, b, gterm, out, M, L, st);
    case 2: return token_head_multi_fwd_launch<2>(ms, nb, W, b, gterm, out, M, L, st);
    case 3: return token_head_multi_fwd_launch<3>(ms, nb, W, b, gterm, out, M, L, st);
    case 4: return token_head_multi_fwd_launch<4>(ms, nb, W, b, gterm, out, M, L, st);
    case 5: return token_head_multi_fwd_launch<5>(ms, nb, W, b, gterm, out, M, L, st);
    case 6: return token_head_multi_fwd_launch<6>(ms, nb, W, b, gterm, out, M, L, st);
    case 7: return token_head_multi_fwd_launch<7>(ms, nb, W, b, gterm, out, M, L, st);
    case 8: return token_head_multi_fwd_launch<8>(ms, nb, W, b, gterm, out, M, L, st);
    case 9: return token_head_multi_fwd_launch<9>(ms, nb, W, b, gterm, out, M, L, st);
    case 10: return token_head_multi_fwd_launch<10>(ms, nb, W, b, gterm, out, M, L, st);
    case 11: return token_head_multi_fwd_launch<11>(ms, nb, W, b, gterm, out, M, L, st);
    case 12: return token_head_multi_fwd_launch<12>(ms, nb, W, b, gterm, out, M, L, st);
    case 13: return token_head_multi_fwd_launch<13>(ms, nb, W, b, gterm, out, M, L, st);
    case 14: return token_head_multi_fwd_launch<14>(ms, nb, W, b, gterm, out, M, L, st);
    case 15: return token_head_multi_fwd_launch<15>(ms, nb, W, b, gterm, out, M, L, st);
    case 16: return token_head_multi_fwd_launch<16>(ms, nb, W, b, gterm, out, M, L, st);
    default: return (int)hipErrorInvalidValue;
  }
}

// Prediction with a per-residue head: operands as pbx_token_head_multi_fwd (nb = 1 without gterm: those of
// pbx_token_head_fwd) -> labels [M] int32, pmax [M] fp32 and, unless probs is null, probs [M][K] fp32 =
// softmax over the K classes; the logits are not written.  tokens ([M] int64, may be null): a row whose token is
// below min_token gets label -1, pmax 0 and a zero probability row.  No atomics: bitwise repeatable.
PBX_EXPORT int pbx_token_head_calls(const void* const* srcs, int nb, const float* W, const float* b,
                                    const float* gterm, const long long* tokens, int min_token, float* probs,
                                    int* labels, float* pmax, long M, int K, int L, hipStream_t st) {
  MultiSrc ms;
  if (M < 1 || L < 1 || labels == nullptr || pmax == nullptr || !multi_src(srcs, nb, ms))
    return (int)hipErrorInvalidValue;
#define PBX_CALLS_CASE(KK) \
  case KK: return token_head_calls_launch<KK>(ms, nb, W, b, gterm, tokens, min_token, probs, labels, pmax, M, L, st);
  switch (K) {
    PBX_CALLS_CASE(1) PBX_CALLS_CASE(2) PBX_CALLS_CASE(3) PBX_CALLS_CASE(4)
    PBX_CALLS_CASE(5) PBX_CALLS_CASE(6) PBX_CALLS_CASE(7) PBX_CALLS_CASE(8)
    PBX_CALLS_CASE(9) PBX_CALLS_CASE(10) PBX_CALLS_CASE(11) PBX_CALLS_CASE(12)
    PBX_CALLS_CASE(13) PBX_CALLS_CASE(14) PBX_CALLS_CASE(15) PBX_CALLS_CASE(16)
    default: return (int)hipErrorInvalidValue;
  }
#undef PBX_CALLS_CASE
}

// Workgroups of pbx_token_head_eval on M rows (workgroup w owns rows 256 w .. 256 w + 255): the partial rows it writes.
PBX_EXPORT int pbx_token_head_eval_parts(long M) {
  return M < 1 ? 0 : (int)((M + 255) / 256);
}

// Evaluation of a per-residue head: operands as pbx_token_head_calls with y ([M] int64 labels: y < 0 ignored,
// y >= K counted as a bad label) in place of the tokens -> loss_part [nwg] fp32 (the workgroup's sum of the live
// rows' cross-entropy) and cnt_part [nwg][K*K + 2] uint32 (confusion true x predicted, live rows, bad labels),
// nwg = pbx_token_head_eval_parts(M).  The logits are not written.  Integer LDS atomics only: bitwise repeatable.
PBX_EXPORT int pbx_token_head_eval(const void* const* srcs, int nb, const float* W, const float* b,
                                   const float* gterm, const long long* y, float* loss_part, unsigned* cnt_part,
                                   long M, int K, int L, hipStream_t st) {
  MultiSrc ms;
  if (M < 1 || L < 1 || W == nullptr || b == nullptr || y == nullptr || loss_part == nullptr || cnt_part == nullptr ||
      !multi_src(srcs, nb, ms))
    return (int)hipErrorInvalidValue;
#define PBX_EVAL_CASE(KK) \
  case KK: return token_head_eval_launch<KK>(ms, nb, W, b, gterm, y, loss_part, cnt_part, M, L, st);
  switch (K) {
    PBX_EVAL_CASE(1) PBX_EVAL_CASE(2) PBX_EVAL_CASE(3) PBX_EVAL_CASE(4)
    PBX_EVAL_CASE(5) PBX_EVAL_CASE(6) PBX_EVAL_CASE(7) PBX_EVAL_CASE(8)
    PBX_EVAL_CASE(9) PBX_EVAL_CASE(10) PBX_EVAL_CASE(11) PBX_EVAL_CASE(12)
    PBX_EVAL_CASE(13) PBX_EVAL_CASE(14) PBX_EVAL_CASE(15) PBX_EVAL_CASE(16)
    default: return (int)hipErrorInvalidValue;
  }
#undef PBX_EVAL_CASE
}

// One batch's partials of pbx_token_head_eval into the accumulator: acc_loss [1] fp64, acc_cnt [K*K + 4] int64
// (confusion, live rows, bad labels, batches, sequences); one launch, fixed summation order.
PBX_EXPORT int pbx_task_eval_fold(const float* loss_part, const unsigned* cnt_part, int nwg, int K, int n_sequences,
                                  double* acc_loss, long long* acc_cnt, hipStream_t st) {
  if (loss_part == nullptr || cnt_part == nullptr || acc_loss == nullptr || acc_cnt == nullptr || nwg < 1 || K < 1 ||
      K > 16 || n_sequences < 0)
    return (int)hipErrorInvalidValue;
  const int nc = K * K + 2;
  const int rs = nwg >= 16 * 256 ? 16 : (nwg + 255) / 256;     // row ranges of <= 256 partial rows, at most 16 of them
  hipLaunchKernelGGL(task_eval_fold_kernel, dim3(1 + (nc + 15) / 16, rs), dim3(256), 0, st, loss_part, cnt_part, nwg,
                     nc, n_sequences, acc_loss, acc_cnt);
  return pbx_launch_status();
}

// Workgroups of pbx_token_head_loss on M rows (workgroup w owns rows 256 w .. 256 w + 255): the partial rows it writes.
PBX_EXPORT int pbx_token_head_loss_parts(long M) {
  return M < 1 ? 0 : (int)((M + 255) / 256);
}

// Training loss of a per-residue head: operands as pbx_token_head_eval plus cw ([K] fp32 class weights, null:
// all ones) and the label smoothing eps in [0, 1) -> g [M][K] fp32, the unnormalised gradient of the weighted,
// smoothed cross-entropy sum with respect to the logits (zero rows where y < 0 or y >= K; every row < M is
// written), part [nwg][2] fp32 (sum of the rows' losses, sum of their weights) and cnt [nwg][3] uint32 (live
// rows, hits, bad labels), nwg = pbx_token_head_loss_parts(M).  The logits are not written.  No atomics: bitwise
// repeatable.
PBX_EXPORT int pbx_token_head_loss(const void* const* srcs, int nb, const float* W, const float* b,
                                   const float* gterm, const long long* y, const float* cw, float eps, float* g,
                                   float* part, unsigned* cnt, long M, int K, int L, hipStream_t st) {
  MultiSrc ms;
  if (M < 1 || L < 1 || W == nullptr || b == nullptr || y == nullptr || g == nullptr || part == nullptr ||
      cnt == nullptr || !(eps >= 0.f && eps < 1.f) || !multi_src(srcs, nb, ms))
    return (int)hipErrorInvalidValue;
#define PBX_LOSS_CASE(KK) \
  case KK: return token_head_loss_launch<KK>(ms, nb, W, b, gterm, y, cw, eps, g, part, cnt, M, L, st);
  switch (K) {
    PBX_LOSS_CASE(1) PBX_LOSS_CASE(2) PBX_LOSS_CASE(3) PBX_LOSS_CASE(4)
    PBX_LOSS_CASE(5) PBX_LOSS_CASE(6) PBX_LOSS_CASE(7) PBX_LOSS_CASE(8)
    PBX_LOSS_CASE(9) PBX_LOSS_CASE(10) PBX_LOSS_CASE(11) PBX_LOSS_CASE(12)
    PBX_LOSS_CASE(13) PBX_LOSS_CASE(14) PBX_LOSS_CASE(15) PBX_LOSS_CASE(16)
    default: return (int)hipErrorInvalidValue;
  }
#undef PBX_LOSS_CASE
}

// One batch's partials of pbx_token_head_loss -> out [3] fp32 (mean loss = sum loss / sum w, 1 / sum w, accuracy
// = hits / max(1, live); nan and 0 for the first two when sum w == 0) and acc_cnt [3] int64 += (live, hits, bad);
// one launch, fp64 sums in a fixed order.
PBX_EXPORT int pbx_token_head_loss_fold(const float* part, const unsigned* cnt, int nwg, float* out,
                                        long long* acc_cnt, hipStream_t st) {
  if (part == nullptr || cnt == nullptr || out == nullptr || acc_cnt == nullptr || nwg < 1)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(token_head_loss_fold_kernel, dim3(1), dim3(256), 0, st, part, cnt, nwg, out, acc_cnt);
  return pbx_launch_status();
}

// slab: [P][K][nb*128] fp32 partials (P = number of workgroups, chosen by the caller); srcs as above; K <= 16
PBX_EXPORT int pbx_token_head_multi_wgrad(const void* const* srcs, int nb, const float* g, float* slab, long M,
                                          int K, int P, hipStream_t st) {
  MultiSrc ms;
  if (M < 1 || K < 1 || K > 16 || P < 1 || !multi_src(srcs, nb, ms)) return (int)hipErrorInvalidValue;
  if (K <= 8)
    hipLaunchKernelGGL(token_head_multi_wgrad_kernel<8>, dim3(P), dim3(256), 0, st, ms, nb, g, slab, M, K);
  else
    hipLaunchKernelGGL(token_head_multi_wgrad_kernel<16>, dim3(P), dim3(256), 0, st, ms, nb, g, slab, M, K);
  return pbx_launch_status();
}

// out [M][K] fp32 = h [M][128] bf16 . W^T ([K][128] fp32) + b (K <= 16)
PBX_EXPORT int pbx_token_head_fwd(const void* h, const float* W, const float* b, float* out, long M, int K,
                                  hipStream_t st) {
  if (M < 1) return (int)hipErrorInvalidValue;
  switch (K) {
    case 1: return token_head_fwd_launch<1>(h, W, b, out, M, st);
    case 2: return token_head_fwd_launch<2>(h, W, b, out, M, st);
    case 3: return token_head_fwd_launch<3>(h, W, b, out, M, st);
    case 4: return token_head_fwd_launch<4>(h, W, b, out, M, st);
    case 5: return token_head_fwd_launch<5>(h, W, b, out, M, st);
    case 6: return token_head_fwd_launch<6>(h, W, b, out, M, st);
    case 7: return token_head_fwd_launch<7>(h, W, b, out, M, st);
    case 8: return token_head_fwd_launch<8>(h, W, b, out, M, st);
    case 9: return token_head_fwd_launch<9>(h, W, b, out, M, st);
    case 10: return token_head_fwd_launch<10>(h, W, b, out, M, st);
    case 11: return token_head_fwd_launch<11>(h, W, b, out, M, st);
    case 12: return token_head_fwd_launch<12>(h, W, b, out, M, st);
    case 13: return token_head_fwd_launch<13>(h, W, b, out, M, st);
    case 14: return token_head_fwd_launch<14>(h, W, b, out, M, st);
    case 15: return token_head_fwd_launch<15>(h, W, b, out, M, st);
    case 16: return token_head_fwd_launch<16>(h, W, b, out, M, st);
    default: return (int)hipErrorInvalidValue;
  }
}

// slab: [P][K][128] fp32 partials (P = number of workgroups, chosen by the caller); K <= 16
PBX_EXPORT int pbx_token_head_wgrad(const void* h, const float* g, float* slab, long M, int K, int P,
                                    hipStream_t st) {
  if (K < 1 || K > 16 || P < 1) return (int)hipErrorInvalidValue;
  if (K <= 8)
    hipLaunchKernelGGL(token_head_wgrad_kernel<8>, dim3(P), dim3(256), 0, st, (const bf16_t*)h, g, slab, M, K);
  else
    hipLaunchKernelGGL(token_head_wgrad_kernel<16>, dim3(P), dim3(256), 0, st, (const bf16_t*)h, g, slab, M, K);
  return pbx_launch_status();
}

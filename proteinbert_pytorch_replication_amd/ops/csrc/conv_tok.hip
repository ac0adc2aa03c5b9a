// First-block conv forward through token tables (no MFMA).
//
// The first block's input is x[b][pos] = bf16(emb[tok[b][pos]]): at most 32 distinct rows (V = 26 in the
// model).  Both k=9 convolutions (dilation 1 and d) are therefore sums of nine table rows each,
//
//   pre_c[b][pos][co] = bias_c[co] + sum_{k=0..8} T_c[k][ tok[b][pos + (k-4) d_c] ][co]
//   T_c[k][v][co]     = sum_ci bf16(W_c[co][ci][k]) * bf16(emb[v][ci])          (fp32, ci ascending)
//
// with an all-zero row V for taps outside the sequence: 18 row lookups + 18 adds per output element instead of
// the 1,152 MACs conv_fwd3 (conv2.hip, pbx_conv_fwd3t) spends on it.  What remains is conv_fwd3's epilogue,
// reproduced operation by operation: pre rounded to bf16, gelu_n, s1 = x + GELU(pre_n) + GELU(pre_w) + gb
// without FMA contraction, the LayerNorm partial from the stored (rounded) values.  The only numerical
// difference is the order of the fp32 sum inside pre.
//
//   conv_tok_tables : one thread per (conv, tap, row, co), once per step (weights and embedding change every
//                     step); reads the forward fragment images pack_batch built and the bf16 embedding mirror
//                     -- the operand values conv_fwd3 multiplies.
//   conv_fwd_tok    : persistent, one 16-wave workgroup per CU.  Both convs x 128 channels of fp32 tables do
//                     not fit in LDS, so a workgroup owns a 64-channel half (2 x 9 x (V+1) x 256 B = 124 KB at
//                     V = 26), staged once, and walks (sample, 128-position tile) units.  16 lanes x 16 B per
//                     position: a table row is exactly 256 B, so every ds_read_b128 lane group covers all 64
//                     banks whichever tokens its positions hold.  Inside the walk the waves never meet: wave w
//                     owns positions 8 w .. 8 w + 7 of every tile, stages their tokens (+- 4 d halo) as row
//                     byte offsets in an LDS strip of its own and writes its own LayerNorm partial: no
//                     barrier, no cross-wave reduction.  The kernel is VALU-bound (85 % VALU issue,
//                     profiles/r9/conv_tok_counters.txt): what pays is fewer VALU instructions per output.
//
// LayerNorm partials: one (mean, M2) per (sample, tile, channel half, wave) at [B][L / 4][2].  An 8-position x
// 64-channel partial counts as many elements as 4 positions x 128 channels, so the consumers' Chan merge
// takes it as (T1, BM1) = (L / 4, 4); this needs L % 128 == 0, otherwise the launcher declines.
#include "mfma.h"

using namespace pbx;
typedef unsigned short bf16_t;

namespace {
constexpr int CH = 128;
constexpr int HC = 64;                // channels per workgroup
constexpr int BM = 128;               // positions per unit
constexpr int KS = 9;
constexpr int MAXHALO = 20;           // 4 x dilation, dilation <= 5
constexpr int NT = 1024;              // threads per workgroup
constexpr int WP = BM / (NT / 64);     // positions per wave and tile
constexpr int WTOK = WP + 2 * MAXHALO; // tokens a wave stages per tile

// tab: [half 2][conv 2][tap 9][V + 1][64] fp32; row V is the zero row
__global__ void __launch_bounds__(256) conv_tok_tables_kernel(const bf16x8* __restrict__ fwn,
                                                              const bf16x8* __restrict__ fww,
                                                              const bf16_t* __restrict__ emb, float* __restrict__ tab,
                                                              int V) {
  const int R = V + 1;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= 2 * KS * R * CH) return;
  const int co = idx & 127;
  int r = idx >> 7;
  const int v = r % R;
  r /= R;
  const int k = r % KS, c = r / KS;
  float acc = 0.f;
  if (v < V) {
    const bf16x8* fw = c ? fww : fwn;
    // forward image (conv2.hip): fragment (k * 8 + kb) * 4 + mb, lane (co & 31) + 32 h holds ci = 16 kb + 8 h + j
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const uint4 wq = *reinterpret_cast<const uint4*>(fw + (size_t)(((k * 8 + (q >> 1)) * 4 + (co >> 5)) * 64 +
                                                                     (co & 31) + 32 * (q & 1)));
      const uint4 eq = *reinterpret_cast<const uint4*>(emb + (size_t)v * CH + q * 8);
      float wv[8], ev[8];
      unpack8(wq, wv);
      unpack8(eq, ev);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc = fmaf(wv[j], ev[j], acc);
    }
  }
  tab[((size_t)(((co >> 6) * 2 + c) * KS + k) * R + v) * HC + (co & 63)] = acc;
}

__device__ __forceinline__ f32x2 lo2(const float4& v) { return (f32x2){v.x, v.y}; }
__device__ __forceinline__ f32x2 hi2(const float4& v) { return (f32x2){v.z, v.w}; }

// two fp32 -> one dword of two bf16 (RNE, as f2bf) in ONE v_cvt_pk_bf16_f32: the kernel is VALU-bound
// (profiles/r9/conv_tok_counters.txt) and the scalar casts of packq4 / packq8 did not pair up here (a convert
// and a shift or a byte-select OR per value)
__device__ __forceinline__ unsigned pk2(const f32x2& v) {
  typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
}
__device__ __forceinline__ f32x2 unpk2(unsigned q) {
  return (f32x2){__uint_as_float(q << 16), __uint_as_float(q & 0xffff0000u)};
}

// STORE: write GELU'(pre) of both convs for the backward (training forward).  DIL: the wide conv's dilation at
// compile time (the model's 5: its nine token reads then cost no address arithmetic) or 0 for the argument
template <bool STORE, int DIL>
__global__ void __launch_bounds__(NT) conv_fwd_tok_kernel(
    const long long* __restrict__ tok, const bf16_t* __restrict__ emb, const float* __restrict__ tab,
    const float* __restrict__ bn, const float* __restrict__ bw, const float* __restrict__ gb,
    bf16_t* __restrict__ pre_n, bf16_t* __restrict__ pre_w, bf16_t* __restrict__ s1, float* __restrict__ stats,
    int B, int L, int dil_arg, int V) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int R = V + 1;
  const int RS = R * 256;                                     // bytes of one (conv, tap) table
  unsigned char* tabs = smem;                                 // [2][9][R] rows of 64 fp32
  unsigned char* xe = tabs + 2 * KS * RS;                     // [R] rows of 64 bf16 (this half of emb)
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  float* bias = reinterpret_cast<float*>(xe + R * 128);       // bn | bw of this half (re-read per pass: the
                                                              // rows in flight leave no registers to hold them)
  int* wt = reinterpret_cast<int*>(bias + 2 * HC) + w * WTOK; // this wave's table row byte offsets
  const int hf = blockIdx.x & 1;
  const int T = L / BM, NU = B * T;
  const int nwg = gridDim.x >> 1;
  const int dil = DIL ? DIL : dil_arg;
  const int halo = 4 * dil;
  const int c4 = tid & 15, q = lane >> 4;                     // 16-B chunk of the 64-channel row, position
  const int wtoks = WP + 2 * halo;
  const int ch0 = hf * HC + c4 * 4;

  // the token at index i - halo of this wave's positions of unit u as a table row offset (zero row outside the
  // sequence or the vocabulary)
  auto tok_off = [&](int u, int i) {
    const int b = u / T, pos = (u - b * T) * BM + w * WP - halo + i;
    int v = V;
    if (pos >= 0 && pos < L) {
      const long long t = tok[(size_t)b * L + pos];
      v = (t >= 0 && t < V) ? (int)t : V;
    }
    return v << 8;
  };

  int u = blockIdx.x >> 1;
  {
    const uint4* src = reinterpret_cast<const uint4*>(tab + (size_t)hf * 2 * KS * R * HC);
    stage_chunks(
        2 * KS * R * 16, [&](int idx) { return src[idx]; },
        [&](int idx, uint4 v) { *reinterpret_cast<uint4*>(tabs + idx * 16) = v; });
    for (int idx = tid; idx < R * 8; idx += NT) {
      const int v = idx >> 3;
      const uint4 xr = v < V ? *reinterpret_cast<const uint4*>(emb + (size_t)v * CH + hf * HC + (idx & 7) * 8)
                             : make_uint4(0u, 0u, 0u, 0u);
      *reinterpret_cast<uint4*>(xe + idx * 16) = xr;
    }
  }
  int tcur = u < NU && lane < wtoks ? tok_off(u, lane) : 0;
  if (tid < 2 * HC) bias[tid] = tid < HC ? bn[hf * HC + tid] : bw[hf * HC + tid - HC];
  float4 gbv = u < NU ? *reinterpret_cast<const float4*>(gb + (size_t)(u / T) * CH + ch0) : make_float4(0.f, 0.f, 0.f, 0.f);
  __syncthreads();

  for (; u < NU; u += nwg) {
    const int b = u / T, t = u - b * T;
    const int un = u + nwg;
    // a wave's LDS accesses complete in issue order, so the strip needs no workgroup barrier: the fences only
    // keep the compiler from moving the strip's reads across its write
    if (lane < wtoks) wt[lane] = tcur;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // the next unit's tokens and gb row are in flight during this unit
    float4 gbn = gbv;
    if (un < NU && lane < wtoks) tcur = tok_off(un, lane);
    if (un < NU) gbn = *reinterpret_cast<const float4*>(gb + (size_t)(un / T) * CH + ch0);
    const f32x2 gbp[2] = {lo2(gbv), hi2(gbv)};
    f32x2 sum2 = {0.f, 0.f}, sq2 = {0.f, 0.f};                         // sums / sums of squares, two lanes each
#pragma unroll 1
    for (int ps = 0; ps < 2; ++ps) {
      const int p = w * WP + ps * 4 + q;
      const int* to = wt + halo + ps * 4 + q;
      const unsigned char* tb = tabs + c4 * 16;
      // all 18 row offsets, then all 18 row reads in flight at once (left to itself the compiler chains
      // read -> wait -> add and exposes the LDS latency 18 times), then the rows summed tap by tap in fp32
      // (packed adds: two channels per instruction)
      int on[KS], ow[KS];
#pragma unroll
      for (int k = 0; k < KS; ++k) {
        on[k] = to[k - 4];
        ow[k] = to[(k - 4) * dil];
      }
      float4 rn[KS], rw[KS];
#pragma unroll
      for (int k = 0; k < KS; ++k) rn[k] = *reinterpret_cast<const float4*>(tb + k * RS + on[k]);
#pragma unroll
      for (int k = 0; k < KS; ++k) rw[k] = *reinterpret_cast<const float4*>(tb + (KS + k) * RS + ow[k]);
      __builtin_amdgcn_sched_barrier(0);
      f32x2 an[2] = {lo2(rn[0]), hi2(rn[0])}, aw[2] = {lo2(rw[0]), hi2(rw[0])};
#pragma unroll
      for (int k = 1; k < KS; ++k) {
        an[0] += lo2(rn[k]);
        an[1] += hi2(rn[k]);
      }
#pragma unroll
      for (int k = 1; k < KS; ++k) {
        aw[0] += lo2(rw[k]);
        aw[1] += hi2(rw[k]);
      }
      const uint2 xq = *reinterpret_cast<const uint2*>(xe + (to[0] >> 1) + c4 * 8);
      const float4 bnv = *reinterpret_cast<const float4*>(bias + c4 * 4);
      const float4 bwv = *reinterpret_cast<const float4*>(bias + HC + c4 * 4);
      an[0] += lo2(bnv); an[1] += hi2(bnv);
      aw[0] += lo2(bwv); aw[1] += hi2(bwv);
      // pre rounded to bf16 as conv_fwd3 stages it, then the build's GELU core on the rounded values
      const f32x2 gi[4] = {unpk2(pk2(an[0])), unpk2(pk2(an[1])), unpk2(pk2(aw[0])), unpk2(pk2(aw[1]))};
      const f32x2 xv[2] = {unpk2(xq.x), unpk2(xq.y)};
      f32x2 go[4];
      // byte offset of this thread's 4 channels: 32 bits (the launcher bounds B L), so the three stores take
      // the uniform base + 32-bit offset form
      const unsigned off = (((unsigned)b * L + t * BM + p) * CH + ch0) * 2;
      if constexpr (STORE) {
        f32x2 gd[4];
        gelu_n<4, 2>(gi, go, gd);
        *reinterpret_cast<uint2*>(reinterpret_cast<unsigned char*>(pre_n) + off) = make_uint2(pk2(gd[0]), pk2(gd[1]));
        *reinterpret_cast<uint2*>(reinterpret_cast<unsigned char*>(pre_w) + off) = make_uint2(pk2(gd[2]), pk2(gd[3]));
      } else {
        gelu_n<4, 0>(gi, go, nullptr);
      }
      uint2 oq;
      {
        // the order and the absence of FMA contraction of conv_fwd3 / conv_fwd5
#pragma clang fp contract(off)
        oq.x = pk2(xv[0] + go[0] + go[2] + gbp[0]);
        oq.y = pk2(xv[1] + go[1] + go[3] + gbp[1]);
      }
      *reinterpret_cast<uint2*>(reinterpret_cast<unsigned char*>(s1) + off) = oq;
      // the LayerNorm partial from the stored (rounded) values
      const f32x2 r0 = unpk2(oq.x), r1 = unpk2(oq.y);
      sum2 += r0;
      sum2 += r1;
      sq2 = __builtin_elementwise_fma(r0, r0, sq2);
      sq2 = __builtin_elementwise_fma(r1, r1, sq2);
    }
    {
      const float sa = wave_reduce_sum(sum2.x + sum2.y), sq = wave_reduce_sum(sq2.x + sq2.y);
      if (lane == 0) {
        const float n = (float)(WP * HC), m = sa / n;
        float* dst = stats + (((size_t)b * T + t) * (2 * NT / 64) + hf * (NT / 64) + w) * 2;
        dst[0] = m;
        dst[1] = fmaxf(sq - sa * m, 0.f);
      }
    }
    gbv = gbn;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

int tok_lds(int V) { return 2 * KS * (V + 1) * 256 + (V + 1) * 128 + 2 * HC * 4 + (NT / 64) * WTOK * 4; }

int num_cus() {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 2)
      n = 256;
    cus = n;
  }
  return cus;
}
}  // namespace

// 1 when pbx_conv_fwd_tok takes this shape (otherwise the caller keeps pbx_conv_fwd3t)
PBX_EXPORT int pbx_conv_fwd_tok_ok(int B, int L, int KS_, int dil, int V) {
  return B >= 1 && L >= BM && L % BM == 0 && KS_ == KS && dil >= 1 && 4 * dil <= MAXHALO && V >= 1 && V <= 32 &&
         tok_lds(V) <= 163840 && (long long)B * L < (1ll << 24);   // 32-bit byte offsets into [B][L][128] bf16
}

// tab: 2 x 2 x 9 x (V + 1) x 64 floats, from the forward fragment images of the narrow / wide conv weights
// (pbx_pack_conv_frag / pbx_pack_batch) and the bf16 embedding [V][128]
PBX_EXPORT int pbx_conv_tok_tables(const void* fwn, const void* fww, const void* emb, float* tab, int V,
                                   hipStream_t st) {
  if (V < 1 || V > 32) return (int)hipErrorInvalidValue;
  const int n = 2 * KS * (V + 1) * CH;
  hipLaunchKernelGGL(conv_tok_tables_kernel, dim3((n + 255) / 256), dim3(256), 0, st, (const bf16x8*)fwn,
                     (const bf16x8*)fww, (const bf16_t*)emb, tab, V);
  return pbx_launch_status();
}

// The first block's conv forward from the tables: tok [B][L] int64 in [0, V), emb [V][128] bf16, the other
// arguments as pbx_conv_fwd3t, except stats: [B][L / 4][2], to be read with (T1, BM1) = (L / 4, 4).
PBX_EXPORT int pbx_conv_fwd_tok(const long long* tok, const void* emb, const float* tab, const float* bn,
                                const float* bw, const float* gb, void* pre_n, void* pre_w, void* s1, float* stats,
                                int B, int L, int KS_, int dil, int V, hipStream_t st) {
  if (!pbx_conv_fwd_tok_ok(B, L, KS_, dil, V) || tok == nullptr || emb == nullptr || tab == nullptr || gb == nullptr ||
      (pre_n == nullptr) != (pre_w == nullptr))
    return (int)hipErrorInvalidValue;
  static bool attrs_set = false;
  if (!attrs_set) {
    for (const void* k : {(const void*)conv_fwd_tok_kernel<true, 5>, (const void*)conv_fwd_tok_kernel<false, 5>,
                          (const void*)conv_fwd_tok_kernel<true, 0>, (const void*)conv_fwd_tok_kernel<false, 0>})
      (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 163840);
    attrs_set = true;
  }
  const int NU = B * (L / BM);
  int grid = num_cus() & ~1;
  if (grid > 2 * NU) grid = 2 * NU;
  const auto kern = dil == 5 ? (pre_n != nullptr ? conv_fwd_tok_kernel<true, 5> : conv_fwd_tok_kernel<false, 5>)
                             : (pre_n != nullptr ? conv_fwd_tok_kernel<true, 0> : conv_fwd_tok_kernel<false, 0>);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(NT), tok_lds(V), st, tok, (const bf16_t*)emb, tab, bn, bw, gb,
                     (bf16_t*)pre_n, (bf16_t*)pre_w, (bf16_t*)s1, stats, B, L, dil, V);
  return pbx_launch_status();
}

// Attention maps of the paper-semantics global attention: the softmax weights themselves, for every head of
// up to 8 blocks in one launch pair.  pa_fused_fwd_kernel (paper_fused.hip) keeps them in LDS for one tile and
// stores only o and lse; here they are the output:
//
//   s[b,h,l] = sum_k qs[b,h,k] tanh(h2[b,l,:] . Wk[h][:,k]),  p[b,h,:] = softmax of s over the live positions
//
// with the operands of the encoder's own attention: qs = tanh(g Wq) / sqrt(K) in fp32 (pbx_sg_query_fwd), the
// bf16 key rows of pbx_pa_wimg, bf16 h2, fp32 MFMA accumulation, the pad mask.
//
// pbx_attn_map_scores: workgroup = 8 waves x 32 positions (one 256-position chunk of one sample of one block),
// lane = position.  There is no value projection, so a head's LDS image is its 64 key rows (16 KB) and ALL heads
// of a block (H <= 8: 128 KB) stay in LDS: h2 is read once per block whatever H.  The key tile is that of
// pa_fused_fwd_kernel: D[k][pos] (A = Wk^T rows from LDS, B = h2 row fragments), the score reduces over k inside
// the lane with one exchange across the half-waves.  Every in-range raw score goes straight into the output
// tensor (-inf where masked) and a (max, sum exp) partial is written per (row, chunk).  The walk is persistent
// and grid-stride over (block, sample, chunk) items, block-major, and a workgroup restages the key image only
// when the block changes.
//
// pbx_attn_map_normalize: one wave per (b, block, h) row merges the chunk partials in ascending chunk order (as
// pa_fused_combine_kernel) and rewrites the row in place as exp(s - M) / sum: +0.0 at a masked position, a row
// without a live position all zeros.
//
// A row's bits depend on that row's h2, qs, mask, the weights and L only: a position's score is one MFMA column
// (columns do not mix), the partials are per (row, chunk) in a fixed order, and there are no atomics.
#include "mfma.h"

using namespace pbx;
typedef unsigned short bf16_t;

namespace {
constexpr int CH = 128;
constexpr int PK = 64;                 // key dim
constexpr int NW = 8;                  // waves per workgroup
constexpr int CHUNK = 32 * NW;         // positions per work item
constexpr int MAXH = 8;                // heads whose key rows fit in LDS together
constexpr int MAXBLK = 8;              // blocks per launch
constexpr int HBYTES = PK * 256;       // one head's key image

struct MapSrc {
  const bf16_t* h2[MAXBLK];            // [B, L, 128] bf16
  const bf16_t* wk[MAXBLK];            // [H][64][128] bf16: row k of head h is Wk[h][:, k]
  const float* qs[MAXBLK];             // [B, H, 64] fp32
};

// the encoder's own tanh (tanh_fast of paper_fused.hip): saturates correctly at +-inf
__device__ __forceinline__ float tanh_fast(float x) {
  const float e = __expf(2.0f * x);
  return 1.0f - 2.0f * __builtin_amdgcn_rcpf(e + 1.0f);
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// out [B][NB][H][L] fp32 (rows of blocks blk0 .. blk0 + nb - 1 written); part [B*NB*H][nchunk][2] fp32
__global__ void __launch_bounds__(64 * NW) attn_map_scores_kernel(MapSrc src, const unsigned char* __restrict__ mask,
                                                                  float* __restrict__ out, float* __restrict__ part,
                                                                  int B, int L, int H, int nb, int blk0, int NB) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* ws = smem;                                          // [H][64 rows][256 B], swizzled
  float* qsl = reinterpret_cast<float*>(smem + H * HBYTES);          // [H][64]
  float* mrg = qsl + H * PK;                                         // [NW][H][2]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int nchunk = (L + CHUNK - 1) / CHUNK;
  const long per_blk = (long)B * nchunk;
  const long items = per_blk * nb;
  int staged = -1;
  for (long item = blockIdx.x; item < items; item += gridDim.x) {
    const int blk = (int)(item / per_blk);
    const long rem = item - (long)blk * per_blk;
    const int b = (int)(rem / nchunk), c = (int)(rem - (long)b * nchunk);
    __syncthreads();                                                 // previous item's LDS readers done
    if (blk != staged) {
      const bf16_t* wimg = src.wk[blk];
      stage_chunks(
          H * PK * 16, [&](int idx) { return *reinterpret_cast<const uint4*>(wimg + (size_t)idx * 8); },
          [&](int idx, uint4 v) { *reinterpret_cast<uint4*>(ws + swz256(idx >> 4, idx & 15)) = v; });
      staged = blk;
    }
    if (tid < H * PK) qsl[tid] = src.qs[blk][(size_t)b * H * PK + tid];
    __syncthreads();
    const int pos = c * CHUNK + w * 32 + r;
    const int posc = min(pos, L - 1);
    const bool inb = pos < L;
    const bool okp = inb && (mask == nullptr || mask[(size_t)b * L + posc] != 0);
    // h2 row fragments of this lane's position (half h: channels kk*16 + 8h .. +8); zeros past the end
    bf16x8 hf[8];
    {
      const bf16_t* row = src.h2[blk] + ((size_t)b * L + posc) * CH;
#pragma unroll
      for (int kk = 0; kk < 8; ++kk) {
        const uint4 v = *reinterpret_cast<const uint4*>(row + kk * 16 + 8 * h);
        hf[kk] = __builtin_bit_cast(bf16x8, inb ? v : make_uint4(0u, 0u, 0u, 0u));
      }
    }
    float* orow = out + (((size_t)b * NB + blk0 + blk) * H) * (size_t)L;
#pragma unroll 1
    for (int j = 0; j < H; ++j) {
      float sp = 0.f;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
        f32x16_t ka = zero16();
#pragma unroll
        for (int kk = 0; kk < 8; ++kk)
          ka = mfma32(lds_frag(ws, swz256(j * PK + kb * 32 + r, kk * 2 + h)), hf[kk], ka);
        // ka[4g + e] = D[k = kb*32 + 8g + 4h + e][pos]
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const float4 q4 = *reinterpret_cast<const float4*>(qsl + j * PK + kb * 32 + 8 * g + 4 * h);
          sp += q4.x * tanh_fast(ka[4 * g]) + q4.y * tanh_fast(ka[4 * g + 1]) + q4.z * tanh_fast(ka[4 * g + 2]) +
                q4.w * tanh_fast(ka[4 * g + 3]);
        }
      }
      const float s = okp ? sp + __shfl_xor(sp, 32, 64) : -INFINITY;
      if (h == 0 && inb) orow[(size_t)j * L + pos] = s;
      const float m = wave_max(s);
      const float p = (okp && m > -INFINITY) ? __expf(s - m) : 0.f;
      const float l = wave_reduce_sum(h == 0 ? p : 0.f);
      if (lane == 0) {
        mrg[(w * H + j) * 2] = m;
        mrg[(w * H + j) * 2 + 1] = l;
      }
    }
    __syncthreads();
    if (tid < H) {                                                   // thread j merges head j over the NW waves
      const int j = tid;
      float M = -INFINITY;
#pragma unroll
      for (int ww = 0; ww < NW; ++ww) M = fmaxf(M, mrg[(ww * H + j) * 2]);
      float Ls = 0.f;
#pragma unroll
      for (int ww = 0; ww < NW; ++ww) {
        const float mw = mrg[(ww * H + j) * 2];
        const float cw = (mw == -INFINITY) ? 0.f : __expf(mw - M);
        Ls = fmaf(mrg[(ww * H + j) * 2 + 1], cw, Ls);
      }
      float* pp = part + ((((size_t)b * NB + blk0 + blk) * H + j) * nchunk + c) * 2;
      pp[0] = M;
      pp[1] = Ls;
    }
  }
}

// one wave per (b, i, h) row of the launch's nb blocks
__global__ void __launch_bounds__(64) attn_map_normalize_kernel(float* __restrict__ out, const float* __restrict__ part,
                                                                int L, int H, int nb, int blk0, int NB, int nchunk) {
  const int lane = threadIdx.x;
  const long rid = blockIdx.x;                                       // over (b, i, h)
  const int hh = (int)(rid % H);
  const long bi = rid / H;
  const int i = (int)(bi % nb);
  const long b = bi / nb;
  const size_t row = ((size_t)b * NB + blk0 + i) * H + hh;
  const float* p = part + row * nchunk * 2;
  float M = -INFINITY;
  for (int k = 0; k < nchunk; ++k) M = fmaxf(M, p[2 * k]);
  float Ls = 0.f;
  for (int k = 0; k < nchunk; ++k) {
    const float c = (p[2 * k] == -INFINITY) ? 0.f : __expf(p[2 * k] - M);
    Ls = fmaf(p[2 * k + 1], c, Ls);
  }
  float* o = out + row * (size_t)L;
  if (Ls > 0.f) {
    for (int l = lane; l < L; l += 64) o[l] = __expf(o[l] - M) / Ls;   // exp(-inf) = +0.0 at a masked position
  } else {
    for (int l = lane; l < L; l += 64) o[l] = 0.f;                     // no live position
  }
}

int g_am_cus = -1;
int am_num_cus() {
  if (g_am_cus < 0) {
    int dev = 0;
    g_am_cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) {
      hipDeviceProp_t p;
      if (hipGetDeviceProperties(&p, dev) == hipSuccess) g_am_cus = p.multiProcessorCount;
    }
  }
  return g_am_cus;
}
bool g_am_attrs = false;
int am_lds(int H) { return H * HBYTES + (H * PK + NW * H * 2) * 4; }
// workgroups per CU: 16 waves (two workgroups) fit the 128-register kernel; the LDS image (16.3 KB per head)
// fits twice up to H = 4
int am_wgs_per_cu(int H) { return 2 * am_lds(H) <= 160 * 1024 ? 2 : 1; }
bool am_src(const void* const* p, int nb) {
  if (p == nullptr) return false;
  for (int i = 0; i < nb; ++i)
    if (p[i] == nullptr || (reinterpret_cast<uintptr_t>(p[i]) & 15) != 0) return false;   // 16-B loads
  return true;
}
bool am_args(int B, int L, int H, int nb, int blk0, int NB) {
  return B >= 1 && L >= 1 && H >= 1 && H <= MAXH && nb >= 1 && nb <= MAXBLK && blk0 >= 0 && NB >= 1 &&
         (long)blk0 + nb <= NB;
}
}  // namespace

// The most workgroups a pbx_attn_map_scores launch of H heads uses (CUs x workgroups per CU): with more
// (block, sample, chunk) items than this its workgroups walk several.
PBX_EXPORT int pbx_attn_map_grid_cap(int H) {
  if (H < 1 || H > MAXH) return 0;
  return am_num_cus() * am_wgs_per_cu(H);
}

// Raw scores and per-chunk softmax partials of blocks blk0 .. blk0 + nb - 1 (nb <= 8) of an NB-block map.
// h2s / wks / qss: HOST arrays of the nb device addresses (h2_i [B, L, 128] bf16; the key image of block i,
// [H][64][128] bf16 as pbx_pa_wimg writes it with VD = 0; qs_i [B, H, 64] fp32), all 16-byte aligned.
// mask [B, L] u8 or null.  out [B][NB][H][L] fp32: every element of the launch's rows is written (-inf where
// masked); part [B*NB*H][ceil(L/256)][2] fp32: (max, sum exp) of every (row, chunk) of those rows.  1 <= H <= 8.
PBX_EXPORT int pbx_attn_map_scores(const void* const* h2s, const void* const* wks, const void* const* qss,
                                   const void* mask, float* out, float* part, int B, int L, int H, int nb, int blk0,
                                   int NB, hipStream_t st) {
  if (!am_args(B, L, H, nb, blk0, NB) || out == nullptr || part == nullptr || !am_src(h2s, nb) || !am_src(wks, nb) ||
      !am_src(qss, nb))
    return (int)hipErrorInvalidValue;
  if (!g_am_attrs) {
    (void)hipFuncSetAttribute((const void*)attn_map_scores_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 163840);
    g_am_attrs = true;
  }
  MapSrc src;
  for (int i = 0; i < MAXBLK; ++i) {
    const int s = i < nb ? i : 0;
    src.h2[i] = (const bf16_t*)h2s[s];
    src.wk[i] = (const bf16_t*)wks[s];
    src.qs[i] = (const float*)qss[s];
  }
  const long nchunk = (L + CHUNK - 1) / CHUNK;
  const long items = (long)nb * B * nchunk;
  long grid = pbx_attn_map_grid_cap(H);
  if (grid > items) grid = items;
  hipLaunchKernelGGL(attn_map_scores_kernel, dim3((unsigned)grid), dim3(64 * NW), am_lds(H), st, src,
                     (const unsigned char*)mask, out, part, B, L, H, nb, blk0, NB);
  return pbx_launch_status();
}

// out rows of blocks blk0 .. blk0 + nb - 1: raw scores -> softmax weights, in place, from the partials of
// pbx_attn_map_scores on the same arguments.
PBX_EXPORT int pbx_attn_map_normalize(float* out, const float* part, int B, int L, int H, int nb, int blk0, int NB,
                                      hipStream_t st) {
  if (!am_args(B, L, H, nb, blk0, NB) || out == nullptr || part == nullptr) return (int)hipErrorInvalidValue;
  const long rows = (long)B * nb * H;
  if (rows > 0x7fffffffL) return (int)hipErrorInvalidValue;
  const int nchunk = (L + CHUNK - 1) / CHUNK;
  hipLaunchKernelGGL(attn_map_normalize_kernel, dim3((unsigned)rows), dim3(64), 0, st, out, part, L, H, nb, blk0, NB,
                     nchunk);
  return pbx_launch_status();
}

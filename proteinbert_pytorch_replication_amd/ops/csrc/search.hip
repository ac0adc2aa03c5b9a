// Embedding search (ops/search.py): the k best database rows of every query by inner product, streamed.
//
//   pbx_search_topk   Q [nq][D] bf16, X [n][D] bf16 -> per query and per split of the database the first k
//                     candidates of the total order (score descending, then index ascending), and optionally
//                     every score.  The [nq][n] score matrix exists only when the caller asks for it.
//
// Score: s[q][r] = sum_d float(Q[q][d]) * float(X[r][d]), accumulated in fp32 on v_mfma_f32_32x32x16_bf16 from a
// zero accumulator, the k-steps in ascending d.  Every (q, r) goes through the same instruction sequence whatever
// the grid, the split count or its place in a tile, so a score's bits depend on the two rows alone.
//
// Shape of the kernel: a workgroup of 4 waves owns 128 queries (32 per wave, their operand fragments resident
// in registers: D / 16 fragments of 4 VGPRs) and one split of the database.  It streams the split in tiles of
// 32 rows, staged through LDS in chunks of up to 512 columns (one chunk per tile up to D = 512, two above) and
// shared by the four waves.  Two chunk images in LDS and two register sets: while chunk s is multiplied, chunk
// s + 1 is on its way from the registers to LDS and the global loads of chunk s + 2 are in flight, so a load has
// a whole chunk's time and more before it is waited for.  The database rows are the A operand, the queries the
// B operand: a lane holds one query (column lane & 31) and 16 of the tile's 32 rows.
//
// Selection: each query's best k live in LDS as an unordered set with its worst member (lowest score, among
// equal scores the highest index) tracked as the threshold.  A tile in which some score beats its query's
// threshold takes the candidate path: the passing scores go to a wave-private LDS image, and the lane that owns
// a query walks that query's passing rows in ASCENDING ROW ORDER, replacing the worst member each time.  One lane
// per query, rows in index order: no counter, no atomic, nothing depends on which lane met a candidate first.
// At the end every list is ranked by the total order and stored.  Every output element is written by exactly one
// thread with a plain store.
#include "mfma.h"

#include <float.h>
#include <limits.h>

using namespace pbx;
typedef unsigned short bf16_t;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));   // 16 bytes in flight between global memory and LDS

namespace {
constexpr int TR = 32;            // database rows per tile
constexpr int QW = 32;            // queries per wave
constexpr int NW = 4;             // waves per workgroup
constexpr int QT = QW * NW;       // queries per workgroup
constexpr int KC = 512;           // columns per staged chunk (32 k-steps)
constexpr int NP = TR * (KC / 8) / 256;   // 16-B pieces of a chunk image per thread
constexpr int MAXK = 64;
constexpr int GS = 16;            // list members per group: a group's worst member is cached
constexpr int NG = MAXK / GS;
constexpr int MAX_MERGE = 256 * 64;   // pbx_row_topk's widest row: S * k may not exceed it

// LDS: two chunk images of TR rows (row pitch = chunk bytes + 16: the 16 rows of a ds_read_b128 lane group
// then start on 16 distinct 16-B slots), one 32 x 32 fp32 candidate image per wave, the lists [k][QW] per wave,
// and per wave the groups' worst members (score, index, slot) [NG][QW].
__host__ __device__ inline int chunk_cols(int D) { return D < KC ? D : KC; }
__host__ __device__ inline int row_pitch(int D) { return chunk_cols(D) * 2 + 16; }
inline size_t lds_bytes(int D, int k) {
  return (size_t)2 * TR * row_pitch(D) + (size_t)NW * TR * QW * 4 + (size_t)NW * k * QW * 8 +
         (size_t)NW * NG * QW * 12;
}

__device__ __forceinline__ void wave_sync_lds() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ long lmin(long a, long b) { return a < b ? a : b; }

// row of the tile held by accumulator register `reg` of a lane in half h (fragment map of csrc/mfma.h)
__device__ __forceinline__ int acc_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

// NDMAX: the most k-steps (D / 16) this instance takes: the query fragments are a register array.  Up to 32
// k-steps a tile is one chunk; the 64-step instance takes 512 < D <= 1024 as two chunks per tile.  Up to D = 128
// the registers are held to 256 so that two workgroups share a CU and hide each other's load latency.
template <int NDMAX>
__global__ void __launch_bounds__(256, NDMAX <= 8 ? 2 : 1) search_topk_kernel(const bf16_t* __restrict__ Q, long ldq,
                                                          const bf16_t* __restrict__ X, long ldx, int nq, int n, int D,
                                                          int k, int S, int nqt, int tps, float* __restrict__ pval,
                                                          int* __restrict__ pidx, float* __restrict__ scores, long lds,
                                                          int order) {
  constexpr int NCH = NDMAX > 32 ? 2 : 1;        // chunks per tile
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int nd = D >> 4;
  const int cpr = chunk_cols(D) >> 3;            // 16-B pieces per staged row
  const int pitch = row_pitch(D);
  unsigned char* xb = smem;
  float* scr = reinterpret_cast<float*>(smem + 2 * TR * pitch) + w * TR * QW;
  float* lv = reinterpret_cast<float*>(smem + 2 * TR * pitch + NW * TR * QW * 4) + w * k * QW;
  int* li = reinterpret_cast<int*>(smem + 2 * TR * pitch + NW * TR * QW * 4 + NW * k * QW * 4) + w * k * QW;
  unsigned char* gbase = smem + 2 * TR * pitch + NW * TR * QW * 4 + NW * k * QW * 8;
  float* gv = reinterpret_cast<float*>(gbase) + w * NG * QW;
  int* gi = reinterpret_cast<int*>(gbase + NW * NG * QW * 4) + w * NG * QW;
  int* gp = reinterpret_cast<int*>(gbase + NW * NG * QW * 8) + w * NG * QW;

  // order 0: the query tile is the fastest-varying index (workgroups on one database range run together)
  const int bid = (int)blockIdx.x;
  const int qt = order == 0 ? bid % nqt : bid / S;
  const int sp = order == 0 ? bid / nqt : bid % S;
  const int T = (int)(((long)n + TR - 1) / TR);
  const int tb = min(sp * tps, T), te = min(tb + tps, T);     // S * tps < T + S: no overflow

  const int q0 = qt * QT + w * QW;
  const bool wact = q0 < nq;                     // wave-uniform: a wave without queries only stages
  bf16x8 bq[NDMAX];
  {
    const long qrow = min(q0 + r, nq - 1);       // clamped: queries past nq repeat the last one, never stored
    const bf16_t* qp = Q + qrow * ldq + 8 * h;
#pragma unroll
    for (int i = 0; i < NDMAX; ++i) {
      if (wact && i < nd) bq[i] = *reinterpret_cast<const bf16x8*>(qp + i * 16);
      else bq[i] = __builtin_bit_cast(bf16x8, make_uint4(0u, 0u, 0u, 0u));
    }
  }

  // staging map: this thread moves pieces tid + 256 j (j < NP) of a chunk image, piece = (row, 16-B column).
  // Stage s of the split is chunk s % NCH of tile tb + s / NCH.
  int srow[NP], sch[NP];
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const int idx = tid + 256 * j;
    srow[j] = idx / cpr;
    sch[j] = idx - srow[j] * cpr;
  }
  const int ns = (te - tb) * NCH;
  auto issue = [&](u32x4* v, int s) __attribute__((always_inline)) {
    const int t = tb + (NCH == 2 ? s >> 1 : s), c = NCH == 2 ? (s & 1) : 0;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      const int col = c * KC + sch[j] * 8;
      if (srow[j] < TR && col < D) {
        const long gr = lmin((long)t * TR + srow[j], (long)n - 1);   // rows past n: a clamped, valid address
        v[j] = *reinterpret_cast<const u32x4*>(X + gr * ldx + col);
      }
    }
  };
  auto commit = [&](const u32x4* v, int buf, int s) __attribute__((always_inline)) {
    const int c = NCH == 2 ? (s & 1) : 0;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      if (srow[j] < TR && c * KC + sch[j] * 8 < D)
        *reinterpret_cast<u32x4*>(xb + buf * TR * pitch + srow[j] * pitch + sch[j] * 16) = v[j];
    }
  };

  // list state of query q0 + lane (lanes < 32); thr is kept on both lanes of a query
  int cnt = 0, wpos = 0;
  float thr = -INFINITY;                         // below every finite score until the list is full
  f32x16_t acc = zero16();

  auto multiply = [&](int buf, int c) __attribute__((always_inline)) {          // c: compile-time at every call site
    if (!wact) return;
    const unsigned char* xt = xb + buf * TR * pitch + r * pitch + h * 16;
#pragma unroll
    for (int kk = 0; kk < KC / 16; ++kk) {
      const int i = c * (KC / 16) + kk;
      if (i < NDMAX && i < nd) acc = mfma32(lds_frag(xt, kk * 32), bq[i < NDMAX ? i : 0], acc);
    }
  };

  // The worst member of this lane's full list: lowest score, then highest index.  The list is kept in groups of
  // GS members whose worst one is cached, so a replacement rescans one group (its loads are independent and
  // issued together) and compares the groups' worst.  Slots past k repeat the last one, which changes nothing.
  auto scan_group = [&](int g) __attribute__((always_inline)) {
    float wv = INFINITY;
    int wi = -1, wp = 0;
    for (int u0 = 0; u0 < GS; u0 += 8) {
      float tv[8];
      int ti[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int j = min(g * GS + u0 + u, k - 1);
        tv[u] = lv[j * QW + lane];
        ti[u] = li[j * QW + lane];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        if (tv[u] < wv || (tv[u] == wv && ti[u] > wi)) {
          wv = tv[u];
          wi = ti[u];
          wp = min(g * GS + u0 + u, k - 1);
        }
      }
    }
    gv[g * QW + lane] = wv;
    gi[g * QW + lane] = wi;
    gp[g * QW + lane] = wp;
  };
  auto pick_worst = [&]() __attribute__((always_inline)) {
    const int ng = (k + GS - 1) / GS;
    float wv = INFINITY;
    int wi = -1, wp = 0;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const int gg = min(g, ng - 1);
      const float v = gv[gg * QW + lane];
      const int i = gi[gg * QW + lane], p = gp[gg * QW + lane];
      if (v < wv || (v == wv && i > wi)) {
        wv = v;
        wi = i;
        wp = p;
      }
    }
    wpos = wp;
    thr = wv;
  };

  auto select = [&](int t) __attribute__((always_inline)) {                     // the scores of tile t are in acc
    if (!wact) return;
    const long rb = (long)t * TR;
    const int nvalid = (int)lmin((long)TR, (long)n - rb);     // rows of this tile that exist
    if (scores != nullptr && q0 + r < nq) {
      float* so = scores + (long)(q0 + r) * lds + rb;
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int i = acc_row(reg, h);
        if (i < nvalid) so[i] = acc[reg];
      }
    }
    // A split streams its rows in ascending order, so once a query's list is full every later row with a score
    // EQUAL to the list's worst has a larger index than all members and loses the tie: a strict > against the
    // threshold is exact.  (While the list fills, thr = -inf admits every finite score.)
    unsigned m = 0;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int i = acc_row(reg, h);
      if (i < nvalid && acc[reg] > thr) m |= 1u << i;
    }
    if (!__any(m != 0)) return;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int i = acc_row(reg, h);
      if ((m >> i) & 1u) scr[i * QW + r] = acc[reg];
    }
    wave_sync_lds();
    unsigned rm = m | (unsigned)__shfl_xor((int)m, 32, 64);   // the passing rows of query r, from both halves
    if (lane < QW) {
      while (rm != 0) {                          // ascending rows: the order of the database, not of arrival
        const int i = __ffs(rm) - 1;
        rm &= rm - 1;
        const float s = scr[i * QW + lane];
        if (s > thr) {                           // strict, against the threshold as the rows before this one left it
          const bool full = cnt == k;
          const int slot = full ? wpos : cnt;
          lv[slot * QW + lane] = s;
          li[slot * QW + lane] = (int)(rb + i);
          cnt = full ? k : cnt + 1;
          if (cnt == k) {
            // a replacement changed one group; the list just filled: every group is scanned for the first time
            const int g0 = full ? slot / GS : 0, g1 = full ? g0 + 1 : (k + GS - 1) / GS;
            for (int g = g0; g < g1; ++g) scan_group(g);
            pick_worst();
          }
        }
      }
    }
    wave_sync_lds();
    thr = __shfl(thr, r, 64);
  };

  // prologue: chunks 0 and 1 on their way, chunk 0 in LDS
  u32x4 va[NP], vb[NP];
  if (ns > 0) issue(va, 0);
  if (ns > 1) issue(vb, 1);
  if (ns > 0) commit(va, 0, 0);
  __syncthreads();
  for (int s = 0; s < ns; s += 2) {              // every condition below is workgroup-uniform
    // even chunk: image 0.  va is free (chunk s left it), vb holds chunk s + 1
    if (s + 2 < ns) issue(va, s + 2);
    multiply(0, 0);
    if (s + 1 < ns) commit(vb, 1, s + 1);
    __syncthreads();
    if (NCH == 1) {
      select(tb + s);
      acc = zero16();
    }
    if (s + 1 >= ns) break;
    // odd chunk: image 1.  vb is free, va holds chunk s + 2
    if (s + 3 < ns) issue(vb, s + 3);
    multiply(1, NCH == 2 ? 1 : 0);
    if (s + 2 < ns) commit(va, 0, s + 2);
    __syncthreads();
    select(NCH == 2 ? tb + (s >> 1) : tb + s + 1);
    acc = zero16();
  }

  if (!wact) return;
  wave_sync_lds();
  // rank every list by (score descending, index ascending): lane j ranks member j of one query at a time
  for (int qq = 0; qq < QW; ++qq) {
    const int qi = q0 + qq;
    if (qi >= nq) break;                         // wave-uniform
    const int c = __shfl(cnt, qq, 64);
    float myv = -FLT_MAX;
    int myi = INT_MAX, rank = lane;              // free slots: -FLT_MAX / INT32_MAX at their own place
    if (lane < c) {
      myv = lv[lane * QW + qq];
      myi = li[lane * QW + qq];
      rank = 0;
      for (int j = 0; j < c; ++j) {
        const float ov = lv[j * QW + qq];
        const int oi = li[j * QW + qq];
        rank += (ov > myv || (ov == myv && oi < myi)) ? 1 : 0;
      }
    }
    if (lane < k) {
      const long o = ((long)qi * S + sp) * k + rank;
      pval[o] = myv;
      pidx[o] = myi;
    }
  }
}

template <int NDMAX>
int search_launch(const bf16_t* Q, long ldq, const bf16_t* X, long ldx, int nq, int n, int D, int k, int S, int nqt,
                  int tps, float* pval, int* pidx, float* scores, long lds, int order, hipStream_t st) {
  static bool attr = false;                      // up to 150 KiB of dynamic LDS: above the default limit
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)search_topk_kernel<NDMAX>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds_bytes(1024, MAXK));
    attr = true;
  }
  hipLaunchKernelGGL(search_topk_kernel<NDMAX>, dim3((unsigned)(nqt * S)), dim3(256), lds_bytes(D, k), st, Q, ldq, X,
                     ldx, nq, n, D, k, S, nqt, tps, pval, pidx, scores, lds, order);
  return pbx_launch_status();
}
}  // namespace

// Q [nq][ldq] bf16, X [n][ldx] bf16 (D columns used, D a multiple of 16 in 16 .. 1024; rows 16-byte aligned),
// 1 <= k <= min(64, n), splits S >= 1 with S * k <= 16384 (the limits ops/search.search_supported publishes)
// -> pval [nq][S][k] fp32, pidx [nq][S][k] int32: split j covers a contiguous run of whole 32-row tiles and
// holds the first k of (score descending, index ascending) over it, free slots -FLT_MAX / INT32_MAX.
// scores: null, or fp32 [nq][lds] (lds >= n): every score of the launch, the bits the selection used.
// order: 0 = query tile fastest in the grid, 1 = split fastest.  Scores must be finite.
PBX_EXPORT int pbx_search_topk(const void* Q, long ldq, const void* X, long ldx, int nq, int n, int D, int k,
                               int splits, float* pval, int* pidx, float* scores, long lds, int order,
                               hipStream_t st) {
  if (Q == nullptr || X == nullptr || pval == nullptr || pidx == nullptr) return (int)hipErrorInvalidValue;
  if (nq < 1 || n < 1 || D < 16 || D > 1024 || (D & 15) != 0) return (int)hipErrorInvalidValue;
  if (k < 1 || k > MAXK || k > n || splits < 1 || (long)splits * k > MAX_MERGE) return (int)hipErrorInvalidValue;
  if (ldq < D || ldx < D || (ldq & 7) != 0 || (ldx & 7) != 0) return (int)hipErrorInvalidValue;
  if ((((uintptr_t)Q) & 15) != 0 || (((uintptr_t)X) & 15) != 0) return (int)hipErrorInvalidValue;
  if ((scores != nullptr && lds < n) || (order != 0 && order != 1)) return (int)hipErrorInvalidValue;
  const long nqt = ((long)nq + QT - 1) / QT;
  if (nqt * splits > 0x7fffffffL) return (int)hipErrorInvalidValue;
  const int T = (int)(((long)n + TR - 1) / TR);
  const int tps = (T + splits - 1) / splits;
  const bf16_t* q = (const bf16_t*)Q;
  const bf16_t* x = (const bf16_t*)X;
  auto fn = D <= 128 ? search_launch<8> : D <= 256 ? search_launch<16> : D <= 512 ? search_launch<32>
                                                                                   : search_launch<64>;
  return fn(q, ldq, x, ldx, nq, n, D, k, splits, (int)nqt, tps, pval, pidx, scores, lds, order, st);
}

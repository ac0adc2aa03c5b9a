// Flat-arena optimizer kernels.
//
// The reference runs torch.optim.Adam over 133 tensors (~1,066 foreach kernel
// launches per step).  Here every parameter lives in ONE fp32
// arena, so the whole update is one memory-bound launch (16 B/lane vector
// loads), hyper-parameters are read from device memory (the step is
// hipGraph-capturable), and a device-side "skip" flag drops the update when
// the loss was non-finite without a host sync.  Math is exactly torch Adam
// (non-decoupled weight decay, denom = sqrt(v)/sqrt(bc2) + eps).
#include "common.h"

struct AdamHParams {  // device-resident, float32
  float lr, beta1, beta2, eps, weight_decay, bias_correction1, bias_correction2_sqrt, grad_scale;
};

__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, const AdamHParams& h) {
  g = g * h.grad_scale + h.weight_decay * p;
  m = h.beta1 * m + (1.0f - h.beta1) * g;
  v = h.beta2 * v + (1.0f - h.beta2) * g * g;
  const float denom = sqrtf(v) / h.bias_correction2_sqrt + h.eps;
  p -= (h.lr / h.bias_correction1) * (m / denom);
}

// Optional bf16 shadow (nullptr to skip): written from the updated fp32 master.
// step_dev (optional): device step counter t (already incremented for this step); the bias
// corrections are then computed on the device, so the launch is replayable from a hipGraph.
__global__ void __launch_bounds__(256) adam_flat_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                        float* __restrict__ m, float* __restrict__ v,
                                                        unsigned short* __restrict__ shadow, int64_t n,
                                                        const AdamHParams* __restrict__ hp,
                                                        const int* __restrict__ skip,
                                                        const float* __restrict__ step_dev) {
  if (skip != nullptr && *skip != 0) return;
  AdamHParams h = *hp;
  if (step_dev != nullptr) {
    const float t = *step_dev;
    h.bias_correction1 = 1.0f - powf(h.beta1, t);
    h.bias_correction2_sqrt = sqrtf(1.0f - powf(h.beta2, t));
  }
  const int64_t n4 = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 pp = reinterpret_cast<float4*>(p)[i];
    const float4 gg = reinterpret_cast<const float4*>(g)[i];
    float4 mm = reinterpret_cast<float4*>(m)[i];
    float4 vv = reinterpret_cast<float4*>(v)[i];
    adam_one(pp.x, gg.x, mm.x, vv.x, h);
    adam_one(pp.y, gg.y, mm.y, vv.y, h);
    adam_one(pp.z, gg.z, mm.z, vv.z, h);
    adam_one(pp.w, gg.w, mm.w, vv.w, h);
    reinterpret_cast<float4*>(p)[i] = pp;
    reinterpret_cast<float4*>(m)[i] = mm;
    reinterpret_cast<float4*>(v)[i] = vv;
    if (shadow != nullptr) {
      ushort4 s;
      s.x = f2bf(pp.x); s.y = f2bf(pp.y); s.z = f2bf(pp.z); s.w = f2bf(pp.w);
      reinterpret_cast<ushort4*>(shadow)[i] = s;
    }
  }
  // tail
  const int64_t t = (n4 << 2) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n && blockIdx.x * blockDim.x + threadIdx.x < 4) {
    float pp = p[t], mm = m[t], vv = v[t];
    adam_one(pp, g[t], mm, vv, h);
    p[t] = pp; m[t] = mm; v[t] = vv;
    if (shadow != nullptr) shadow[t] = f2bf(pp);
  }
}

PBX_EXPORT int pbx_adam_flat(float* p, const float* g, float* m, float* v, void* shadow, int64_t n,
                             const void* hparams, const int* skip, const float* step_dev, hipStream_t stream) {
  if (n <= 0) return 0;
  int64_t blocks = ((n >> 2) + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(adam_flat_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, p, g, m, v,
                     (unsigned short*)shadow, n, (const AdamHParams*)hparams, skip, step_dev);
  return pbx_launch_status();
}

// ---- parameter groups ------------------------------------------------------------------------
// Every arena segment starts on a 64-element boundary, so one byte per 64-element block names the
// block's group (block_group, relative to p) and the update stays one launch for any number of
// groups: +1/64 byte per element on top of the ~30 the update moves.  Each workgroup resolves the
// groups' blocks once (device bias corrections from each group's own betas) into LDS; a lane
// reads the block of its group from there.  A wave's 64 lanes cover four 64-element blocks per
// pass, i.e. up to four groups.  Bit k of decoupled_mask: group k decays its weights AdamW's way.
#define PBX_ADAM_MAX_GROUPS 16

// torch.optim.AdamW: p *= 1 - lr * wd first, no wd * p term in the gradient
__device__ __forceinline__ void adam_one_decoupled(float& p, float g, float& m, float& v, const AdamHParams& h) {
  p *= 1.0f - h.lr * h.weight_decay;
  g = g * h.grad_scale;
  m = h.beta1 * m + (1.0f - h.beta1) * g;
  v = h.beta2 * v + (1.0f - h.beta2) * g * g;
  const float denom = sqrtf(v) / h.bias_correction2_sqrt + h.eps;
  p -= (h.lr / h.bias_correction1) * (m / denom);
}

__global__ void __launch_bounds__(256) adam_flat_groups_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                               float* __restrict__ m, float* __restrict__ v,
                                                               unsigned short* __restrict__ shadow, int64_t n,
                                                               const AdamHParams* __restrict__ hp, int n_groups,
                                                               unsigned decoupled_mask,
                                                               const unsigned char* __restrict__ block_group,
                                                               const int* __restrict__ skip,
                                                               const float* __restrict__ step_dev) {
  if (skip != nullptr && *skip != 0) return;
  __shared__ AdamHParams hs[PBX_ADAM_MAX_GROUPS];
  if ((int)threadIdx.x < n_groups) {
    AdamHParams h = hp[threadIdx.x];
    if (step_dev != nullptr) {
      const float t = *step_dev;
      h.bias_correction1 = 1.0f - powf(h.beta1, t);
      h.bias_correction2_sqrt = sqrtf(1.0f - powf(h.beta2, t));
    }
    hs[threadIdx.x] = h;
  }
  __syncthreads();
  const int64_t n4 = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    // 16 float4 per 64-element block; the mask keeps a bad table entry inside hs
    const unsigned gi = block_group[i >> 4] & (PBX_ADAM_MAX_GROUPS - 1);
    const AdamHParams h = hs[gi];
    float4 pp = reinterpret_cast<float4*>(p)[i];
    const float4 gg = reinterpret_cast<const float4*>(g)[i];
    float4 mm = reinterpret_cast<float4*>(m)[i];
    float4 vv = reinterpret_cast<float4*>(v)[i];
    if ((decoupled_mask >> gi) & 1u) {
      adam_one_decoupled(pp.x, gg.x, mm.x, vv.x, h);
      adam_one_decoupled(pp.y, gg.y, mm.y, vv.y, h);
      adam_one_decoupled(pp.z, gg.z, mm.z, vv.z, h);
      adam_one_decoupled(pp.w, gg.w, mm.w, vv.w, h);
    } else {
      adam_one(pp.x, gg.x, mm.x, vv.x, h);
      adam_one(pp.y, gg.y, mm.y, vv.y, h);
      adam_one(pp.z, gg.z, mm.z, vv.z, h);
      adam_one(pp.w, gg.w, mm.w, vv.w, h);
    }
    reinterpret_cast<float4*>(p)[i] = pp;
    reinterpret_cast<float4*>(m)[i] = mm;
    reinterpret_cast<float4*>(v)[i] = vv;
    if (shadow != nullptr) {
      ushort4 s;
      s.x = f2bf(pp.x); s.y = f2bf(pp.y); s.z = f2bf(pp.z); s.w = f2bf(pp.w);
      reinterpret_cast<ushort4*>(shadow)[i] = s;
    }
  }
  // tail
  const int64_t t = (n4 << 2) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n && blockIdx.x * blockDim.x + threadIdx.x < 4) {
    const unsigned gi = block_group[t >> 6] & (PBX_ADAM_MAX_GROUPS - 1);
    const AdamHParams h = hs[gi];
    float pp = p[t], mm = m[t], vv = v[t];
    if ((decoupled_mask >> gi) & 1u) adam_one_decoupled(pp, g[t], mm, vv, h);
    else adam_one(pp, g[t], mm, vv, h);
    p[t] = pp; m[t] = mm; v[t] = vv;
    if (shadow != nullptr) shadow[t] = f2bf(pp);
  }
}

// hparams: [n_groups][8] float32 (AdamHParams per group); block_group: uint8[ceil(n / 64)]
PBX_EXPORT int pbx_adam_flat_groups(float* p, const float* g, float* m, float* v, void* shadow, int64_t n,
                                    const void* hparams, int n_groups, int decoupled_mask,
                                    const void* block_group, const int* skip, const float* step_dev,
                                    hipStream_t stream) {
  if (n_groups < 1 || n_groups > PBX_ADAM_MAX_GROUPS) return (int)hipErrorInvalidValue;
  if (n <= 0) return 0;
  int64_t blocks = ((n >> 2) + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(adam_flat_groups_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, p, g, m, v,
                     (unsigned short*)shadow, n, (const AdamHParams*)hparams, n_groups, (unsigned)decoupled_mask,
                     (const unsigned char*)block_group, skip, step_dev);
  return pbx_launch_status();
}

// ---- global L2 norm of a flat buffer (clip_grad_norm_) --------------------------
// Two passes in one launch sequence: per-block partial sums of squares -> out[blocks],
// then a single-block reduce into out_total[0].  Deterministic (fixed tree).
__global__ void __launch_bounds__(256) sumsq_partial_kernel(const float* __restrict__ x, int64_t n,
                                                            float* __restrict__ partial) {
  __shared__ float red[4];
  float acc = 0.f;
  const int64_t n4 = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const float4 a = reinterpret_cast<const float4*>(x)[i];
    acc += a.x * a.x + a.y * a.y + a.z * a.z + a.w * a.w;
  }
  const int64_t t = (n4 << 2) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n && blockIdx.x * blockDim.x + threadIdx.x < 4) acc += x[t] * x[t];
  acc = wave_reduce_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

__global__ void __launch_bounds__(256) sumsq_final_kernel(const float* __restrict__ partial, int nb,
                                                          float* __restrict__ out) {
  __shared__ float red[4];
  float acc = 0.f;
  for (int i = threadIdx.x; i < nb; i += 256) acc += partial[i];
  acc = wave_reduce_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = red[0] + red[1] + red[2] + red[3];
}

// workspace must hold 1024 floats
PBX_EXPORT int pbx_sumsq_flat(const float* x, int64_t n, float* workspace, float* out, hipStream_t stream) {
  int64_t blocks = ((n >> 2) + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(sumsq_partial_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, x, n, workspace);
  hipLaunchKernelGGL(sumsq_final_kernel, dim3(1), dim3(256), 0, stream, workspace, (int)blocks, out);
  return pbx_launch_status();
}

// ---- non-finite gradient flag (the fused Adam kernel skips the update when it is set) ----------
// One partial pass (per-block "any NaN / Inf", v - v != 0 exactly for those) and a one-block OR:
// replaces torch.isfinite(grad.sum()) (a 70 MB reduction plus five one-element kernels per step).
// Non-finite test: an element is bad when it is NaN / Inf or |x| >= bound (!(|x| < bound) is true for NaN).
// The DP step passes bound = FLT_MAX / world, so no sum of accepted per-rank values can overflow fp32.
__global__ void __launch_bounds__(256) nonfinite_partial_kernel(const float* __restrict__ x, int64_t n, float bound,
                                                                int* __restrict__ partial) {
  __shared__ int red[4];
  bool bad = false;
  const int64_t n4 = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const float4 a = reinterpret_cast<const float4*>(x)[i];
    const float m = fmaxf(fmaxf(fabsf(a.x), fabsf(a.y)), fmaxf(fabsf(a.z), fabsf(a.w)));   // NaN-free max
    bad |= !(m < bound) || (a.x != a.x) || (a.y != a.y) || (a.z != a.z) || (a.w != a.w);
  }
  const int64_t t = (n4 << 2) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n && blockIdx.x * blockDim.x + threadIdx.x < 4) bad |= !(fabsf(x[t]) < bound);
  const int wb = __any(bad) ? 1 : 0;
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = wb;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0] | red[1] | red[2] | red[3];
}

__global__ void __launch_bounds__(256) nonfinite_final_kernel(const int* __restrict__ partial, int nb,
                                                              int* __restrict__ flag, int accumulate) {
  __shared__ int red[4];
  int acc = 0;
  for (int i = threadIdx.x; i < nb; i += 256) acc |= partial[i];
  const int bad = __any(acc != 0) ? 1 : 0;
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = bad;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int v = red[0] | red[1] | red[2] | red[3];
    flag[0] = accumulate ? (flag[0] | v) : v;
  }
}

// workspace must hold 1024 ints; flag: one int32, set to (accumulate: OR-ed with) 1 when any element of x
// is NaN / Inf or has |x| >= bound (bound = FLT_MAX: exactly the non-finite test)
PBX_EXPORT int pbx_nonfinite_flag(const float* x, int64_t n, int* workspace, int* flag, float bound, int accumulate,
                                  hipStream_t stream) {
  int64_t blocks = ((n >> 2) + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(nonfinite_partial_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, x, n, bound, workspace);
  hipLaunchKernelGGL(nonfinite_final_kernel, dim3(1), dim3(256), 0, stream, workspace, (int)blocks, flag, accumulate);
  return pbx_launch_status();
}

// x *= min(1, max_norm / (sqrt(sumsq) + 1e-6))   (torch.nn.utils.clip_grad_norm_ semantics)
__global__ void __launch_bounds__(256) clip_scale_kernel(float* __restrict__ x, int64_t n,
                                                         const float* __restrict__ sumsq, float max_norm) {
  const float norm = sqrtf(*sumsq);
  const float c = max_norm / (norm + 1e-6f);
  if (c >= 1.0f) return;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) x[i] *= c;
}

PBX_EXPORT int pbx_clip_scale_flat(float* x, int64_t n, const float* sumsq, float max_norm, hipStream_t stream) {
  int64_t blocks = (n + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(clip_scale_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, x, n, sumsq, max_norm);
  return pbx_launch_status();
}

// x[0 .. n) = v (the gradient arena's per-step zero fill: 16-B stores, grid-stride)
__global__ void __launch_bounds__(256) fill_flat_kernel(float* __restrict__ x, int64_t n, float v) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t n4 = n >> 2;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride)
    reinterpret_cast<float4*>(x)[i] = make_float4(v, v, v, v);
  const int64_t t = (n4 << 2) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n && blockIdx.x * blockDim.x + threadIdx.x < 4) x[t] = v;
}

PBX_EXPORT int pbx_fill_flat(float* x, int64_t n, float v, hipStream_t stream) {
  if (n <= 0) return 0;
  if (((uintptr_t)x & 15) != 0) return (int)hipErrorInvalidValue;
  int64_t blocks = (n / 4 + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(fill_flat_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, x, n, v);
  return pbx_launch_status();
}

// *x += v on the device (the optimizer's step counter; one lane, a vector store)
__global__ void __launch_bounds__(64) add_scalar_kernel(float* __restrict__ x, float v) {
  if (threadIdx.x == 0) x[0] = x[0] + v;
}

PBX_EXPORT int pbx_add_scalar(float* x, float v, hipStream_t stream) {
  hipLaunchKernelGGL(add_scalar_kernel, dim3(1), dim3(64), 0, stream, x, v);
  return pbx_launch_status();
}

// *x += v for an int64 device counter (the synthetic-data step counter)
__global__ void __launch_bounds__(64) add_i64_kernel(long long* __restrict__ x, long long v) {
  if (threadIdx.x == 0) x[0] = x[0] + v;
}

PBX_EXPORT int pbx_add_i64(long long* x, long long v, hipStream_t stream) {
  hipLaunchKernelGGL(add_i64_kernel, dim3(1), dim3(64), 0, stream, x, v);
  return pbx_launch_status();
}

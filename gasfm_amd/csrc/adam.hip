// Adam over every parameter tensor of the model in ONE launch, gfx950.
//
// train.py (:97-100) steps torch.optim.Adam after every batch.  torch's fused multi-tensor Adam
// walks the ~880 parameter tensors (145 M values) in ~34 launches of 3-4 us set-up each and reaches
// ~2.9 TB/s (1.39 ms per step, profiles/r5_train_step_breakdown*.txt).  Here a host-built table of
// 4096-value chunks (tensor index, first value) drives one grid: each workgroup updates one chunk of
// one tensor with float4 loads / stores (a scalar tail for sizes that are not multiples of 4),
// reading p, g, m, v and writing p, m, v once: 28 bytes per parameter.
//
// Update (torch.optim.Adam, amsgrad = False, maximize = False; torch/optim/adam.py):
//   g' = g + wd p;  m = m + (1 - b1)(g' - m);  v = b2 v + (1 - b2) g'^2
//   p = p - (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps)
//
// The rest of train.py's step (:133-152) over the same tables, with no atomics and no host reads:
// the global gradient norm (grad_sumsq_kernel: one fp64 partial per chunk; grad_sumsq_finish_kernel:
// the partials in a fixed order), clip_grad_norm_ / clip_grad_value_ in place (grad_clip_kernel), and
// a capturable Adam whose step count, learning rate, loss guard and clip coefficient live on the
// device (adam_control_kernel writes gasfm_adam_ctl, adam_ctl_kernel reads it).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.hpp"

namespace gasfm {
namespace {

constexpr int kT = 256;

struct AdamK {
  float b1, b2, c1, c2, eps, wd, step_size, inv_bc2_sqrt;  // c1 / c2 = 1 - beta1 / 1 - beta2 (rounded from fp64)
};

__device__ __forceinline__ void adam1(float& p, float g, float& m, float& v, const AdamK& k) {
  if (k.wd != 0.f) g = fmaf(k.wd, p, g);
  m = fmaf(k.c1, g - m, m);
  v = fmaf(k.b2, v, k.c2 * g * g);
  const float denom = sqrtf(v) * k.inv_bc2_sqrt + k.eps;
  p = p - k.step_size * (m / denom);
}

// How a gradient value is clipped as it is read (torch's clip_grad_norm_ / clip_grad_value_ applied
// before optimizer.step(), without writing p.grad): g * gscale, or clamp(g, -th, th) in value mode.
// Comparisons, not fminf / fmaxf: a NaN gradient stays NaN, as torch's clamp keeps it.
struct NoClip {
  __device__ __forceinline__ float operator()(float g) const { return g; }
};
struct Clip {
  float gscale, th;
  bool value;
  __device__ __forceinline__ float operator()(float g) const {
    return value ? (g < -th ? -th : (g > th ? th : g)) : g * gscale;
  }
};

// One workgroup's chunk of one tensor: float4 when p, g, m, v are all 16-byte aligned (a scalar tail
// for sizes that are not multiples of 4), scalar otherwise.
template <class G>
__device__ __forceinline__ void adam_chunk(const gasfm_adam_tensor* __restrict__ tensors,
                                           const gasfm_adam_chunk* __restrict__ chunks, const AdamK& k, const G& clip) {
  const gasfm_adam_chunk ch = chunks[blockIdx.x];
  const gasfm_adam_tensor t = tensors[ch.tensor];
  const int64_t end = ch.begin + GASFM_ADAM_CHUNK < t.numel ? ch.begin + GASFM_ADAM_CHUNK : t.numel;
  const bool vec = ((reinterpret_cast<uintptr_t>(t.p) | reinterpret_cast<uintptr_t>(t.g) |
                     reinterpret_cast<uintptr_t>(t.m) | reinterpret_cast<uintptr_t>(t.v)) & 15) == 0;
  if (vec) {
    const int64_t n4 = (end - ch.begin) / 4;
    for (int64_t q = threadIdx.x; q < n4; q += kT) {
      const int64_t i = ch.begin + 4 * q;
      float4 p = *reinterpret_cast<const float4*>(t.p + i);
      const float4 g = *reinterpret_cast<const float4*>(t.g + i);
      float4 m = *reinterpret_cast<const float4*>(t.m + i);
      float4 v = *reinterpret_cast<const float4*>(t.v + i);
      adam1(p.x, clip(g.x), m.x, v.x, k);
      adam1(p.y, clip(g.y), m.y, v.y, k);
      adam1(p.z, clip(g.z), m.z, v.z, k);
      adam1(p.w, clip(g.w), m.w, v.w, k);
      *reinterpret_cast<float4*>(t.p + i) = p;
      *reinterpret_cast<float4*>(t.m + i) = m;
      *reinterpret_cast<float4*>(t.v + i) = v;
    }
    for (int64_t i = ch.begin + 4 * n4 + threadIdx.x; i < end; i += kT)
      adam1(t.p[i], clip(t.g[i]), t.m[i], t.v[i], k);
  } else {
    for (int64_t i = ch.begin + threadIdx.x; i < end; i += kT) adam1(t.p[i], clip(t.g[i]), t.m[i], t.v[i], k);
  }
}

__global__ __launch_bounds__(kT) void adam_kernel(const gasfm_adam_tensor* __restrict__ tensors,
                                                  const gasfm_adam_chunk* __restrict__ chunks, AdamK k) {
  adam_chunk(tensors, chunks, k, NoClip{});
}

// The same update with its step constants, the skip flag and the clip coefficient read from the
// control struct adam_control_kernel wrote earlier on the stream: nothing here depends on a host
// value that changes from step to step, so the launch can be captured.  A skipped step returns
// before any load or store of p, m, v.
__global__ __launch_bounds__(kT) void adam_ctl_kernel(const gasfm_adam_tensor* __restrict__ tensors,
                                                      const gasfm_adam_chunk* __restrict__ chunks,
                                                      const gasfm_adam_ctl* __restrict__ ctl, AdamK k, float th,
                                                      int value_mode) {
  const gasfm_adam_ctl c = *ctl;
  if (c.skip) return;
  k.step_size = c.step_size;
  k.inv_bc2_sqrt = c.inv_bc2_sqrt;
  adam_chunk(tensors, chunks, k, Clip{c.gscale, th, value_mode != 0});
}

// torch's clip coefficient (torch/nn/utils/clip_grad.py): max_norm / (norm + 1e-6) clamped to 1; a
// NaN norm gives a NaN coefficient (the comparison is false), an inf norm 0.
__device__ __forceinline__ float clip_coef(float th, float norm) {
  const float c = th / (norm + 1e-6f);
  return c > 1.f ? 1.f : c;
}

// sum over a workgroup of one fp64 value per thread, in a fixed order: a shuffle-down tree inside
// each wave, then the waves' sums left to right.  The result is valid in thread 0.
template <int T>
__device__ __forceinline__ double block_sum(double acc, double* lds) {
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = acc;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < T / 64; ++w) s += lds[w];
  return s;
}

// partial[chunk] = sum of g^2 over the chunk, accumulated in fp64 (the square of an fp32 value is
// exact in fp64): 4 B read per value.  float4 loads when the gradient pointer is 16-byte aligned (a
// chunk begins at a multiple of 4096 values), scalar loads otherwise.
__global__ __launch_bounds__(kT) void grad_sumsq_kernel(const gasfm_adam_tensor* __restrict__ tensors,
                                                        const gasfm_adam_chunk* __restrict__ chunks,
                                                        double* __restrict__ partial) {
  __shared__ double lds[kT / 64];
  const gasfm_adam_chunk ch = chunks[blockIdx.x];
  const gasfm_adam_tensor t = tensors[ch.tensor];
  const int64_t end = ch.begin + GASFM_ADAM_CHUNK < t.numel ? ch.begin + GASFM_ADAM_CHUNK : t.numel;
  double acc = 0.0;
  int64_t first = ch.begin;
  if ((reinterpret_cast<uintptr_t>(t.g) & 15) == 0) {
    const int64_t n4 = (end - ch.begin) / 4;
    for (int64_t q = threadIdx.x; q < n4; q += kT) {
      const float4 g = *reinterpret_cast<const float4*>(t.g + ch.begin + 4 * q);
      acc = __builtin_fma(double(g.x), double(g.x), acc);
      acc = __builtin_fma(double(g.y), double(g.y), acc);
      acc = __builtin_fma(double(g.z), double(g.z), acc);
      acc = __builtin_fma(double(g.w), double(g.w), acc);
    }
    first += 4 * n4;
  }
  for (int64_t i = first + threadIdx.x; i < end; i += kT) acc = __builtin_fma(double(t.g[i]), double(t.g[i]), acc);
  const double s = block_sum<kT>(acc, lds);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// One workgroup: total = the n partials summed in a fixed order (thread i takes i, i + 1024, ...,
// then block_sum), norm = sqrt(total) rounded to fp32.  n = 0 gives 0.
constexpr int kFinishT = 1024;
__global__ __launch_bounds__(kFinishT) void grad_sumsq_finish_kernel(const double* __restrict__ partial, int64_t n,
                                                                     double* __restrict__ total,
                                                                     float* __restrict__ norm) {
  __shared__ double lds[kFinishT / 64];
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += kFinishT) acc += partial[i];
  const double s = block_sum<kFinishT>(acc, lds);
  if (threadIdx.x == 0) {
    total[0] = s;
    norm[0] = float(__builtin_sqrt(s));
  }
}

// In-place clip of every gradient of the table: g *= clip_coef(th, *norm) (GASFM_CLIP_NORM; torch
// multiplies also when the coefficient is 1) or g = clamp(g, -th, th) (GASFM_CLIP_VALUE).
__global__ __launch_bounds__(kT) void grad_clip_kernel(const gasfm_adam_tensor* __restrict__ tensors,
                                                       const gasfm_adam_chunk* __restrict__ chunks, float th,
                                                       const float* __restrict__ norm) {
  const gasfm_adam_chunk ch = chunks[blockIdx.x];
  const gasfm_adam_tensor t = tensors[ch.tensor];
  const int64_t end = ch.begin + GASFM_ADAM_CHUNK < t.numel ? ch.begin + GASFM_ADAM_CHUNK : t.numel;
  const Clip clip{norm ? clip_coef(th, norm[0]) : 1.f, th, norm == nullptr};
  float* g = const_cast<float*>(t.g);
  int64_t first = ch.begin;
  if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {
    const int64_t n4 = (end - ch.begin) / 4;
    for (int64_t q = threadIdx.x; q < n4; q += kT) {
      float4 x = *reinterpret_cast<const float4*>(g + ch.begin + 4 * q);
      x.x = clip(x.x), x.y = clip(x.y), x.z = clip(x.z), x.w = clip(x.w);
      *reinterpret_cast<float4*>(g + ch.begin + 4 * q) = x;
    }
    first += 4 * n4;
  }
  for (int64_t i = first + threadIdx.x; i < end; i += kT) g[i] = clip(g[i]);
}

// One thread: this step's constants into *ctl from device values only.
__global__ __launch_bounds__(64) void adam_control_kernel(gasfm_adam_ctl* __restrict__ ctl,
                                                          const double* __restrict__ sumsq,
                                                          const float* __restrict__ loss,
                                                          const float* __restrict__ lr_dev, double lr,
                                                          float* __restrict__ step, double beta1, double beta2,
                                                          int norm_mode, float th) {
  if (threadIdx.x != 0) return;
  const bool skip = loss != nullptr && !(loss[0] > 0.f);  // a NaN loss skips, as `if loss.item() > 0` does
  const float t = step[0] + (skip ? 0.f : 1.f);
  if (!skip) step[0] = t;
  const float norm = sumsq ? float(__builtin_sqrt(sumsq[0])) : 0.f;
  if (lr_dev) lr = double(lr_dev[0]);
  // as gasfm_adam_step: bias corrections and step size in fp64, then rounded
  const double bc1 = 1.0 - pow(beta1, double(t));
  const double bc2 = 1.0 - pow(beta2, double(t));
  ctl->skip = skip ? 1 : 0;
  ctl->grad_norm = norm;
  ctl->gscale = norm_mode ? clip_coef(th, norm) : 1.f;
  ctl->step_size = float(lr / bc1);
  ctl->inv_bc2_sqrt = float(1.0 / __builtin_sqrt(bc2));
}

}  // namespace
}  // namespace gasfm

using namespace gasfm;

extern "C" int gasfm_adam_step(const gasfm_adam_tensor* tensors, const gasfm_adam_chunk* chunks, int32_t n_chunks,
                               double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step,
                               void* stream) {
  GASFM_REQUIRE(tensors && chunks && n_chunks > 0 && step > 0, "gasfm_adam_step: n_chunks=%d step=%lld", n_chunks,
                (long long)step);
  GASFM_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0,
                "gasfm_adam_step: betas (%g, %g), eps %g", beta1, beta2, eps);
  // the hyper-parameters arrive as fp64 (torch's python floats): 1 - beta, the bias corrections
  // and the step size in fp64, then rounded (1.f - 0.999f would be 1.3e-5 off)
  const double bc1 = 1.0 - __builtin_pow(beta1, double(step));
  const double bc2 = 1.0 - __builtin_pow(beta2, double(step));
  AdamK k{float(beta1), float(beta2), float(1.0 - beta1), float(1.0 - beta2), float(eps), float(weight_decay),
          float(lr / bc1), float(1.0 / __builtin_sqrt(bc2))};
  hipLaunchKernelGGL(adam_kernel, dim3(n_chunks), dim3(kT), 0, reinterpret_cast<hipStream_t>(stream), tensors, chunks,
                     k);
  return launch_status("gasfm_adam_step");
}

extern "C" int gasfm_grad_sumsq(const gasfm_adam_tensor* tensors, const gasfm_adam_chunk* chunks, int32_t n_chunks,
                                double* partial, void* stream) {
  GASFM_REQUIRE(n_chunks >= 0 && (n_chunks == 0 || (tensors && chunks && partial)), "gasfm_grad_sumsq: n_chunks=%d",
                n_chunks);
  if (n_chunks == 0) return GASFM_OK;
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3(n_chunks), dim3(kT), 0, reinterpret_cast<hipStream_t>(stream), tensors,
                     chunks, partial);
  return launch_status("gasfm_grad_sumsq");
}

extern "C" int gasfm_grad_sumsq_finish(const double* partial, int64_t n, double* total, float* norm, void* stream) {
  GASFM_REQUIRE(n >= 0 && (n == 0 || partial) && total && norm, "gasfm_grad_sumsq_finish: n=%lld", (long long)n);
  hipLaunchKernelGGL(grad_sumsq_finish_kernel, dim3(1), dim3(kFinishT), 0, reinterpret_cast<hipStream_t>(stream),
                     partial, n, total, norm);
  return launch_status("gasfm_grad_sumsq_finish");
}

extern "C" int gasfm_grad_clip(const gasfm_adam_tensor* tensors, const gasfm_adam_chunk* chunks, int32_t n_chunks,
                               int32_t mode, double threshold, const float* norm, void* stream) {
  GASFM_REQUIRE(n_chunks >= 0 && (n_chunks == 0 || (tensors && chunks)), "gasfm_grad_clip: n_chunks=%d", n_chunks);
  GASFM_REQUIRE((mode == GASFM_CLIP_NORM && norm) || mode == GASFM_CLIP_VALUE, "gasfm_grad_clip: mode %d%s", mode,
                mode == GASFM_CLIP_NORM ? " needs the norm" : "");
  if (n_chunks == 0) return GASFM_OK;
  hipLaunchKernelGGL(grad_clip_kernel, dim3(n_chunks), dim3(kT), 0, reinterpret_cast<hipStream_t>(stream), tensors,
                     chunks, float(threshold), mode == GASFM_CLIP_NORM ? norm : nullptr);
  return launch_status("gasfm_grad_clip");
}

extern "C" int gasfm_adam_control(gasfm_adam_ctl* ctl, const double* sumsq, const float* loss, const float* lr_dev,
                                  double lr, float* step, double beta1, double beta2, int32_t clip_mode,
                                  double clip_threshold, void* stream) {
  GASFM_REQUIRE(ctl && step, "gasfm_adam_control: null ctl / step");
  GASFM_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "gasfm_adam_control: betas (%g, %g)",
                beta1, beta2);
  GASFM_REQUIRE(clip_mode >= GASFM_CLIP_NONE && clip_mode <= GASFM_CLIP_VALUE &&
                    (clip_mode != GASFM_CLIP_NORM || sumsq),
                "gasfm_adam_control: clip mode %d%s", clip_mode, clip_mode == GASFM_CLIP_NORM ? " needs sumsq" : "");
  hipLaunchKernelGGL(adam_control_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), ctl, sumsq, loss,
                     lr_dev, lr, step, beta1, beta2, int(clip_mode == GASFM_CLIP_NORM), float(clip_threshold));
  return launch_status("gasfm_adam_control");
}

extern "C" int gasfm_adam_step_ctl(const gasfm_adam_tensor* tensors, const gasfm_adam_chunk* chunks, int32_t n_chunks,
                                   const gasfm_adam_ctl* ctl, double beta1, double beta2, double eps,
                                   double weight_decay, int32_t clip_mode, double clip_threshold, void* stream) {
  GASFM_REQUIRE(tensors && chunks && n_chunks > 0 && ctl, "gasfm_adam_step_ctl: n_chunks=%d", n_chunks);
  GASFM_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0,
                "gasfm_adam_step_ctl: betas (%g, %g), eps %g", beta1, beta2, eps);
  GASFM_REQUIRE(clip_mode >= GASFM_CLIP_NONE && clip_mode <= GASFM_CLIP_VALUE, "gasfm_adam_step_ctl: clip mode %d",
                clip_mode);
  // step_size and inv_bc2_sqrt come from *ctl on the device
  AdamK k{float(beta1), float(beta2), float(1.0 - beta1), float(1.0 - beta2), float(eps), float(weight_decay), 0.f, 0.f};
  hipLaunchKernelGGL(adam_ctl_kernel, dim3(n_chunks), dim3(kT), 0, reinterpret_cast<hipStream_t>(stream), tensors,
                     chunks, ctl, k, float(clip_threshold), int(clip_mode == GASFM_CLIP_VALUE));
  return launch_status("gasfm_adam_step_ctl");
}

// ExpDepthRegularizedOSELoss (code/loss_functions.py:126-150) as sparse per-edge kernels, gfx950.
//
// The reference forms the dense projections Ps @ pts3D ([m, 3, n]) and masks them with the dense
// valid-observation matrix, as its ESFMLoss does (see esfm_loss.hip).  Here, per visibility edge
// e = (c, p) with m_e = values[e] (the normalised measurement):
//   y_e  = P_c [X_p; w_p]                               (3-vector)
//   r_e  = y_xy - y_z * m_e                             (object space error at the predicted depth)
//   l_e  = ||r_e|| + w_reg * exp(-y_z)
//   loss = sum_e l_e / E
//   G_e  = dloss / E * ( r_e / ||r_e|| , -(r_e . m_e) / ||r_e|| - w_reg * exp(-y_z) )
// (the norm's gradient is 0 at r_e = 0, torch's subgradient; the exp term remains), then
// dP_c = sum_{e in c} G_e [X_p; w_p]^T (one workgroup per camera, edges in order) and
// d[X_p; w_p] = sum_{e in p} P_c^T G_e (one thread per point, through the point CSR).
// No gradient hook, no margin: the loss is smooth across the principal plane.
// Deterministic: fixed-order sums, no atomics, no host read.
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "lanes.hpp"

namespace gasfm {
namespace {

constexpr int kT = 256;
constexpr int kSegG = 32;  // workgroups per scene in the segmented sums (as esfm_loss.hip)

__device__ __forceinline__ void ose_project(const float* __restrict__ P, const float* __restrict__ X, int64_t n,
                                            int c, int64_t p, float (&y)[3], float (&xs)[4]) {
  const float* pc = P + int64_t(c) * 12;
  xs[0] = X[p], xs[1] = X[n + p], xs[2] = X[2 * n + p], xs[3] = X[3 * n + p];
#pragma unroll
  for (int i = 0; i < 3; ++i)
    y[i] = fmaf(pc[4 * i], xs[0], fmaf(pc[4 * i + 1], xs[1], fmaf(pc[4 * i + 2], xs[2], pc[4 * i + 3] * xs[3])));
}

// l_e
__device__ __forceinline__ float ose_value(const float (&y)[3], float mx, float my, float w_reg) {
  const float rx = y[0] - y[2] * mx, ry = y[1] - y[2] * my;
  return sqrtf(rx * rx + ry * ry) + w_reg * expf(-y[2]);
}

// G_e; scale = dloss / E
__device__ __forceinline__ void ose_grad(const float (&y)[3], float mx, float my, float w_reg, float scale,
                                         float (&g)[3]) {
  const float rx = y[0] - y[2] * mx, ry = y[1] - y[2] * my;
  const float nr = sqrtf(rx * rx + ry * ry);
  const float s = nr > 0.f ? scale / nr : 0.f;  // d||r||/dr = r / ||r|| (0 at r = 0, as torch)
  g[0] = s * rx;
  g[1] = s * ry;
  g[2] = -s * (rx * mx + ry * my) - scale * w_reg * expf(-y[2]);
}

__device__ __forceinline__ float ose_block_sum(float v, float* sh) {
  v = group_sum<64>(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) sh[wave] = v;
  __syncthreads();
  float s = 0.f;
  for (int w = 0; w < kT / 64; ++w) s += sh[w];
  return s;
}

// part[b] = sum of l_e over workgroup b's grid-stride slice of the edges
__global__ __launch_bounds__(kT) void ose_fwd_kernel(const int32_t* __restrict__ cam, const int32_t* __restrict__ pt,
                                                     const float* __restrict__ vals, int64_t E,
                                                     const float* __restrict__ P, const float* __restrict__ X,
                                                     int64_t n, float w_reg, float* __restrict__ part) {
  __shared__ float sh[kT / 64];
  float s = 0.f;
  for (int64_t e = int64_t(blockIdx.x) * kT + threadIdx.x; e < E; e += int64_t(gridDim.x) * kT) {
    const float2 m = reinterpret_cast<const float2*>(vals)[e];
    float y[3], xs[4];
    ose_project(P, X, n, cam[e], pt[e], y, xs);
    s += ose_value(y, m.x, m.y, w_reg);
  }
  s = ose_block_sum(s, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// dP_c over camera c's contiguous edge range [cptr[c], cptr[c+1]) by the workgroup
__device__ __forceinline__ void ose_cam_grad(const int32_t* __restrict__ cptr, const int32_t* __restrict__ pt,
                                             const float* __restrict__ vals, const float* __restrict__ P,
                                             const float* __restrict__ X, int64_t n, float w_reg, int c, float scale,
                                             float* __restrict__ dP) {
  __shared__ float sh[kT / 64 * 12];
  float acc[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) acc[i] = 0.f;
  for (int e = cptr[c] + threadIdx.x; e < cptr[c + 1]; e += kT) {
    const float2 m = reinterpret_cast<const float2*>(vals)[e];
    float y[3], xs[4], g[3];
    ose_project(P, X, n, c, pt[e], y, xs);
    ose_grad(y, m.x, m.y, w_reg, scale, g);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[4 * i + j] = fmaf(g[i], xs[j], acc[4 * i + j]);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < 12; ++i) acc[i] = group_sum<64>(acc[i]);
  if (lane == 0)
#pragma unroll
    for (int i = 0; i < 12; ++i) sh[wave * 12 + i] = acc[i];
  __syncthreads();
  if (threadIdx.x < 12) {
    float s = 0.f;
    for (int w = 0; w < kT / 64; ++w) s += sh[w * 12 + threadIdx.x];
    dP[int64_t(c) * 12 + threadIdx.x] = s;
  }
}

// d pts3D[:, p] over point p's edges in CSR order (perm: edge ids)
__device__ __forceinline__ void ose_pt_grad(const int32_t* __restrict__ pptr, const int32_t* __restrict__ perm,
                                            const int32_t* __restrict__ cam, const float* __restrict__ vals,
                                            const float* __restrict__ P, const float* __restrict__ X, int64_t n,
                                            float w_reg, int64_t p, float scale, float* __restrict__ dX) {
  float a[4] = {0.f, 0.f, 0.f, 0.f};
  for (int q = pptr[p]; q < pptr[p + 1]; ++q) {
    const int e = perm ? perm[q] : q;
    const float2 m = reinterpret_cast<const float2*>(vals)[e];
    const int c = cam[e];
    float y[3], xs[4], g[3];
    ose_project(P, X, n, c, p, y, xs);
    ose_grad(y, m.x, m.y, w_reg, scale, g);
    const float* pc = P + int64_t(c) * 12;
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] = fmaf(pc[j], g[0], fmaf(pc[4 + j], g[1], fmaf(pc[8 + j], g[2], a[j])));
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) dX[j * n + p] = a[j];
}

__global__ __launch_bounds__(kT) void ose_bwd_cam_kernel(const int32_t* __restrict__ cptr,
                                                         const int32_t* __restrict__ pt,
                                                         const float* __restrict__ vals, int64_t E,
                                                         const float* __restrict__ P, const float* __restrict__ X,
                                                         int64_t n, float w_reg, const float* __restrict__ dloss,
                                                         float* __restrict__ dP) {
  ose_cam_grad(cptr, pt, vals, P, X, n, w_reg, blockIdx.x, dloss[0] / float(E), dP);
}

__global__ __launch_bounds__(kT) void ose_bwd_pt_kernel(const int32_t* __restrict__ pptr,
                                                        const int32_t* __restrict__ perm,
                                                        const int32_t* __restrict__ cam,
                                                        const float* __restrict__ vals, int64_t E,
                                                        const float* __restrict__ P, const float* __restrict__ X,
                                                        int64_t n, float w_reg, const float* __restrict__ dloss,
                                                        float* __restrict__ dX) {
  const int64_t p = int64_t(blockIdx.x) * kT + threadIdx.x;
  if (p >= n) return;
  ose_pt_grad(pptr, perm, cam, vals, P, X, n, w_reg, p, dloss[0] / float(E), dX);
}

// ---- several scenes in one edge list (a union batch), as esfm_loss.hip: scene s owns edges
// [eoff[s], eoff[s+1]); the batch loss is sum_s weight[s] * loss_s; a scene of weight 0 (padding)
// contributes nothing, and its cameras' and points' gradients are exact zeros.

// part[s * kSegG + g] = sum of l_e over scene s's edges, slice g
__global__ __launch_bounds__(kT) void ose_fwd_seg_kernel(const int32_t* __restrict__ cam,
                                                         const int32_t* __restrict__ pt,
                                                         const float* __restrict__ vals,
                                                         const int32_t* __restrict__ eoff,
                                                         const float* __restrict__ P, const float* __restrict__ X,
                                                         int64_t n, float w_reg, float* __restrict__ part) {
  __shared__ float sh[kT / 64];
  const int s = blockIdx.y;
  const int64_t e1 = eoff[s + 1];
  float sum = 0.f;
  for (int64_t e = eoff[s] + int64_t(blockIdx.x) * kT + threadIdx.x; e < e1; e += int64_t(kSegG) * kT) {
    const float2 m = reinterpret_cast<const float2*>(vals)[e];
    float y[3], xs[4];
    ose_project(P, X, n, cam[e], pt[e], y, xs);
    sum += ose_value(y, m.x, m.y, w_reg);
  }
  sum = ose_block_sum(sum, sh);
  if (threadIdx.x == 0) part[int64_t(s) * kSegG + blockIdx.x] = sum;
}

// tot[s] = ordered sum of scene s's kSegG partials; loss = sum over the scenes of weight nonzero of
// weight[s] * tot[s] / E_s, in scene order.  One workgroup, S <= kT.
__global__ __launch_bounds__(kT) void ose_seg_total_kernel(const float* __restrict__ part, int S,
                                                           const int32_t* __restrict__ eoff,
                                                           const float* __restrict__ weight, float* __restrict__ tot,
                                                           float* __restrict__ loss) {
  __shared__ float sh[kT];
  const int s = threadIdx.x;
  if (s < S) {
    float a = 0.f;
    for (int g = 0; g < kSegG; ++g) a += part[int64_t(s) * kSegG + g];
    tot[s] = a;
    sh[s] = a;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float L = 0.f;
    for (int q = 0; q < S; ++q) {
      const float w = weight[q];
      if (w != 0.f) L += w * (sh[q] / float(eoff[q + 1] - eoff[q]));
    }
    loss[0] = L;
  }
}

__global__ __launch_bounds__(kT) void ose_bwd_cam_seg_kernel(
    const int32_t* __restrict__ cptr, const int32_t* __restrict__ pt, const float* __restrict__ vals,
    const int32_t* __restrict__ eoff, const int32_t* __restrict__ scene_of_cam, const float* __restrict__ weight,
    const float* __restrict__ P, const float* __restrict__ X, int64_t n, float w_reg,
    const float* __restrict__ dloss, float* __restrict__ dP) {
  const int c = blockIdx.x;
  const int s = scene_of_cam[c];
  const float w = weight[s];
  if (w == 0.f) {
    if (threadIdx.x < 12) dP[int64_t(c) * 12 + threadIdx.x] = 0.f;
    return;
  }
  ose_cam_grad(cptr, pt, vals, P, X, n, w_reg, c, dloss[0] * w / float(eoff[s + 1] - eoff[s]), dP);
}

__global__ __launch_bounds__(kT) void ose_bwd_pt_seg_kernel(
    const int32_t* __restrict__ pptr, const int32_t* __restrict__ perm, const int32_t* __restrict__ cam,
    const float* __restrict__ vals, const int32_t* __restrict__ eoff, const int32_t* __restrict__ scene_of_pt,
    const float* __restrict__ weight, const float* __restrict__ P, const float* __restrict__ X, int64_t n,
    float w_reg, const float* __restrict__ dloss, float* __restrict__ dX) {
  const int64_t p = int64_t(blockIdx.x) * kT + threadIdx.x;
  if (p >= n) return;
  const int s = scene_of_pt[p];
  const float w = weight[s];
  if (w == 0.f) {
#pragma unroll
    for (int j = 0; j < 4; ++j) dX[j * n + p] = 0.f;
    return;
  }
  ose_pt_grad(pptr, perm, cam, vals, P, X, n, w_reg, p, dloss[0] * w / float(eoff[s + 1] - eoff[s]), dX);
}

}  // namespace
}  // namespace gasfm

using namespace gasfm;

extern "C" int32_t gasfm_ose_part_rows(int64_t E) {
  const int64_t b = (E + kT - 1) / kT;
  return int32_t(b < 1 ? 1 : (b > 1024 ? 1024 : b));
}

extern "C" int gasfm_ose_fwd(const int32_t* cam, const int32_t* pt, const float* vals, int64_t E, const float* P,
                             const float* X, int64_t n, float w_reg, float* part, void* stream) {
  GASFM_REQUIRE(E > 0 && n > 0, "gasfm_ose_fwd: E=%lld n=%lld", (long long)E, (long long)n);
  GASFM_REQUIRE(cam && pt && vals && P && X && part, "gasfm_ose_fwd: null pointer");
  GASFM_REQUIRE((reinterpret_cast<uintptr_t>(vals) & 7) == 0, "gasfm_ose_fwd: vals must be 8-byte aligned");
  hipLaunchKernelGGL(ose_fwd_kernel, dim3(gasfm_ose_part_rows(E)), dim3(kT), 0,
                     reinterpret_cast<hipStream_t>(stream), cam, pt, vals, E, P, X, n, w_reg, part);
  return launch_status("gasfm_ose_fwd");
}

extern "C" int gasfm_ose_bwd(const int32_t* cptr, int32_t m, const int32_t* pptr, const int32_t* perm,
                             const int32_t* cam, const int32_t* pt, const float* vals, int64_t E, const float* P,
                             const float* X, int64_t n, float w_reg, const float* dloss, float* dP, float* dX,
                             void* stream) {
  GASFM_REQUIRE(E > 0 && n > 0 && m > 0, "gasfm_ose_bwd: E=%lld m=%d n=%lld", (long long)E, m, (long long)n);
  GASFM_REQUIRE(cptr && pptr && cam && pt && vals && P && X && dloss && dP && dX, "gasfm_ose_bwd: null pointer");
  GASFM_REQUIRE((reinterpret_cast<uintptr_t>(vals) & 7) == 0, "gasfm_ose_bwd: vals must be 8-byte aligned");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(ose_bwd_cam_kernel, dim3(m), dim3(kT), 0, st, cptr, pt, vals, E, P, X, n, w_reg, dloss, dP);
  hipLaunchKernelGGL(ose_bwd_pt_kernel, dim3(unsigned((n + kT - 1) / kT)), dim3(kT), 0, st, pptr, perm, cam, vals, E,
                     P, X, n, w_reg, dloss, dX);
  return launch_status("gasfm_ose_bwd");
}

extern "C" int32_t gasfm_ose_seg_part_rows(int32_t S) { return S * kSegG; }

extern "C" int gasfm_ose_seg_fwd(const int32_t* cam, const int32_t* pt, const float* vals, const int32_t* eoff,
                                 int32_t S, const float* weight, const float* P, const float* X, int64_t n,
                                 float w_reg, float* part, float* tot, float* loss, void* stream) {
  GASFM_REQUIRE(S > 0 && S <= kT && n > 0, "gasfm_ose_seg_fwd: S=%d n=%lld", S, (long long)n);
  GASFM_REQUIRE(cam && pt && vals && eoff && weight && P && X && part && tot && loss, "gasfm_ose_seg_fwd: null pointer");
  GASFM_REQUIRE((reinterpret_cast<uintptr_t>(vals) & 7) == 0, "gasfm_ose_seg_fwd: vals must be 8-byte aligned");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(ose_fwd_seg_kernel, dim3(kSegG, S), dim3(kT), 0, st, cam, pt, vals, eoff, P, X, n, w_reg, part);
  hipLaunchKernelGGL(ose_seg_total_kernel, dim3(1), dim3(kT), 0, st, part, S, eoff, weight, tot, loss);
  return launch_status("gasfm_ose_seg_fwd");
}

extern "C" int gasfm_ose_seg_bwd(const int32_t* cam_ptr, int32_t m, const int32_t* pt_ptr, const int32_t* perm,
                                 const int32_t* cam, const int32_t* pt, const float* vals, const int32_t* eoff,
                                 int32_t S, const int32_t* scene_of_cam, const int32_t* scene_of_pt,
                                 const float* weight, const float* P, const float* X, int64_t n, float w_reg,
                                 const float* dloss, float* dP, float* dX, void* stream) {
  GASFM_REQUIRE(S > 0 && m > 0 && n > 0, "gasfm_ose_seg_bwd: S=%d m=%d n=%lld", S, m, (long long)n);
  GASFM_REQUIRE(cam_ptr && pt_ptr && cam && pt && vals && eoff && scene_of_cam && scene_of_pt && weight && P && X &&
                    dloss && dP && dX,
                "gasfm_ose_seg_bwd: null pointer");
  GASFM_REQUIRE((reinterpret_cast<uintptr_t>(vals) & 7) == 0, "gasfm_ose_seg_bwd: vals must be 8-byte aligned");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(ose_bwd_cam_seg_kernel, dim3(m), dim3(kT), 0, st, cam_ptr, pt, vals, eoff, scene_of_cam, weight,
                     P, X, n, w_reg, dloss, dP);
  hipLaunchKernelGGL(ose_bwd_pt_seg_kernel, dim3(unsigned((n + kT - 1) / kT)), dim3(kT), 0, st, pt_ptr, perm, cam,
                     vals, eoff, scene_of_pt, weight, P, X, n, w_reg, dloss, dX);
  return launch_status("gasfm_ose_seg_bwd");
}

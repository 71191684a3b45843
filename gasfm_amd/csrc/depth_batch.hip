// The depth branch over a union batch (static_batch.StaticBatch), gfx950: DirectDepthLoss
// (depth_loss.hip), the depth scales and the 2-view error (depth_eval.hip) per scene of a padded
// bucket, so that a depth-head training step captures and replays like the ESFM and OSE steps.
//
// Scene s owns edges [eoff[s], eoff[s+1]); eoff lives on the device.  Every pass runs on the
// (kSegG, S) grid of edge_fwd_seg_kernel: workgroup (g, s) walks the strided slice
// eoff[s] + 256 g + t, + 256 kSegG, ... of scene s and leaves partial row s * kSegG + g;
// seg_total_kernel (edge_loss.hpp) sums a scene's rows in order and, for the loss, the scenes in
// order.  The backward walks the same slices, so it needs no scene-of-edge table.  Launch geometry is a
// function of (E_cap, S) alone; no atomics, no host read; two runs give the same bits.
//   depth_seg_sums    (sum a, sum b) per scene
//   depth_seg_fwd     (sum l_e, sum g_e a_e) per scene with depth_term (depth_term.hpp)
//   depth_seg_bwd     da, elementwise; exact zeros in a scene of weight 0, whose a / b / sums are not read
//   depth_seg_scales  fp64 (sum dp, sum dg) per scene -> float32 means
//   backproj_seg      backproj_edge (depth_edge.hpp) with the scene's rescale factor; (sum, count) per scene
// Streaming passes of 8-12 B per edge (the 2-view error: ~28 B streamed + 20 B gathered): no LDS tiling.
#include "../../include/gasfm_depth_batch.h"
#include "depth_edge.hpp"
#include "depth_term.hpp"
#include "edge_loss.hpp"

static_assert(GASFM_DEPTH_SEG_G == gasfm::kSegG, "gasfm_depth_batch.h and edge_loss.hpp disagree on the slices per scene");

namespace gasfm {
namespace {

// scene s's edge range clamped to [0, E_cap] and its edge count as eoff states it
struct SceneRange {
  int64_t e0, e1;
  float count;
};

__device__ __forceinline__ SceneRange scene_range(const int32_t* __restrict__ eoff, int s, int64_t E_cap) {
  const int64_t a = eoff[s], b = eoff[s + 1];
  SceneRange r;
  r.e0 = a < 0 ? 0 : (a > E_cap ? E_cap : a);
  r.e1 = b < 0 ? 0 : (b > E_cap ? E_cap : b);
  r.count = float(b - a);
  return r;
}

constexpr int64_t kStride = int64_t(kSegG) * kT;

__device__ __forceinline__ void write_part(float (&acc)[2], float* sh, float* __restrict__ part) {
  const float t = block_sums(acc, sh);
  if (threadIdx.x < 2) part[2 * (int64_t(blockIdx.y) * kSegG + blockIdx.x) + threadIdx.x] = t;
}

__global__ __launch_bounds__(kT) void depth_seg_sums_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                            const int32_t* __restrict__ eoff, int64_t E_cap,
                                                            const float* __restrict__ weight,
                                                            float* __restrict__ part) {
  __shared__ float sh[kT / 64 * 2];
  const int s = blockIdx.y;
  float acc[2] = {0.f, 0.f};
  if (weight[s] != 0.f) {  // uniform
    const SceneRange r = scene_range(eoff, s, E_cap);
    for (int64_t e = r.e0 + int64_t(blockIdx.x) * kT + threadIdx.x; e < r.e1; e += kStride) {
      acc[0] += a[e];
      acc[1] += b[e];
    }
  }
  write_part(acc, sh, part);
}

__global__ __launch_bounds__(kT) void depth_seg_fwd_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                           const int32_t* __restrict__ eoff, int64_t E_cap,
                                                           const float* __restrict__ weight,
                                                           const float* __restrict__ sums, int l2,
                                                           float* __restrict__ part) {
  __shared__ float sh[kT / 64 * 2];
  const int s = blockIdx.y;
  float acc[2] = {0.f, 0.f};
  if (weight[s] != 0.f) {
    const SceneRange r = scene_range(eoff, s, E_cap);
    const float Sa = sums[2 * s], Sb = sums[2 * s + 1], k = r.count / (Sa * Sb);
    for (int64_t e = r.e0 + int64_t(blockIdx.x) * kT + threadIdx.x; e < r.e1; e += kStride) {
      float l, g;
      const float ae = a[e];
      depth_term(ae, b[e], Sa, Sb, k, l2, l, g);
      acc[0] += l;
      acc[1] = fmaf(g, ae, acc[1]);
    }
  }
  write_part(acc, sh, part);
}

__global__ __launch_bounds__(kT) void depth_seg_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                           const int32_t* __restrict__ eoff, int64_t E_cap,
                                                           const float* __restrict__ weight,
                                                           const float* __restrict__ sums,
                                                           const float* __restrict__ tot, int l2,
                                                           const float* __restrict__ dloss, float* __restrict__ da) {
  const int s = blockIdx.y;
  const SceneRange r = scene_range(eoff, s, E_cap);
  const float w = weight[s];
  const int64_t first = r.e0 + int64_t(blockIdx.x) * kT + threadIdx.x;
  if (w == 0.f) {
    for (int64_t e = first; e < r.e1; e += kStride) da[e] = 0.f;
    return;
  }
  const float inv_e = 1.f / r.count;
  const float Sa = sums[2 * s], Sb = sums[2 * s + 1], k = r.count / (Sa * Sb), inv_sa = r.count / Sa;
  const float up = dloss[0] * w, ga = tot[2 * s + 1];
  for (int64_t e = first; e < r.e1; e += kStride) {
    float l, g;
    depth_term(a[e], b[e], Sa, Sb, k, l2, l, g);
    // d(a_e / s_a)/da_k = delta_ek / s_a - a_e / (E s_a^2), as depth_bwd_kernel
    da[e] = up * inv_e * inv_sa * (g - ga * inv_e * inv_sa);
  }
}

// ws[s * kSegG + g] = fp64 (sum dp, sum dg) of the slice
__global__ __launch_bounds__(kT) void depth_seg_scale_sums_kernel(const float* __restrict__ dp,
                                                                  const float* __restrict__ dg,
                                                                  const int32_t* __restrict__ eoff, int64_t E_cap,
                                                                  double* __restrict__ ws) {
  __shared__ Sum2 sh[kT];
  const int s = blockIdx.y;
  const SceneRange r = scene_range(eoff, s, E_cap);
  Sum2 v{0.0, 0.0};
  for (int64_t e = r.e0 + int64_t(blockIdx.x) * kT + threadIdx.x; e < r.e1; e += kStride) {
    v.a += double(dp[e]);
    v.b += double(dg[e]);
  }
  v = block_tree(v, sh, sum2_merge);
  if (threadIdx.x == 0) {
    const int64_t row = int64_t(s) * kSegG + blockIdx.x;
    ws[2 * row] = v.a;
    ws[2 * row + 1] = v.b;
  }
}

// scales[s] = float(sum of scene s's rows in order / E_s); no edges: NaN.  One workgroup, S <= kT.
__global__ __launch_bounds__(kT) void depth_seg_scales_kernel(const double* __restrict__ ws, int S,
                                                              const int32_t* __restrict__ eoff,
                                                              float* __restrict__ scales) {
  const int s = threadIdx.x;
  if (s >= S) return;
  double sa = 0.0, sb = 0.0;
  for (int g = 0; g < kSegG; ++g) {
    sa += ws[2 * (int64_t(s) * kSegG + g)];
    sb += ws[2 * (int64_t(s) * kSegG + g) + 1];
  }
  const int64_t n = int64_t(eoff[s + 1]) - int64_t(eoff[s]);
  const float nan = __int_as_float(0x7fc00000);
  scales[2 * s] = n > 0 ? float(sa / double(n)) : nan;
  scales[2 * s + 1] = n > 0 ? float(sb / double(n)) : nan;
}

__global__ __launch_bounds__(kT) void backproj_seg_kernel(const int32_t* __restrict__ cam,
                                                          const int32_t* __restrict__ pt,
                                                          const float* __restrict__ xy, const float* __restrict__ d,
                                                          const float* __restrict__ scales,
                                                          const int32_t* __restrict__ src,
                                                          const int32_t* __restrict__ eoff, int64_t E_cap,
                                                          const float* __restrict__ tab, int32_t m,
                                                          float* __restrict__ err, float* __restrict__ rdepth,
                                                          float* __restrict__ part) {
  __shared__ float sh[kT / 64 * 2];
  const int s = blockIdx.y;
  const SceneRange r = scene_range(eoff, s, E_cap);
  const float scale = scales[2 * s + 1] / scales[2 * s];
  float acc[2] = {0.f, 0.f};
  for (int64_t e2 = r.e0 + int64_t(blockIdx.x) * kT + threadIdx.x; e2 < r.e1; e2 += kStride) {
    float v, z;
    backproj_edge(cam, pt, xy, d, scale, src, E_cap, tab, m, e2, v, z);
    if (err) err[e2] = v;
    if (rdepth) rdepth[e2] = z;
    const bool ok = !isnan(v);
    acc[0] += ok ? v : 0.f;
    acc[1] += ok ? 1.f : 0.f;
  }
  write_part(acc, sh, part);
}

int check_batch(const char* name, const int32_t* eoff, int32_t S, int64_t E_cap) {
  GASFM_REQUIRE(S > 0 && S <= kT && E_cap >= 0 && E_cap <= INT32_MAX, "%s: S=%d E_cap=%lld", name, S,
                (long long)E_cap);
  GASFM_REQUIRE(eoff, "%s: null eoff", name);
  return GASFM_OK;
}

}  // namespace
}  // namespace gasfm

using namespace gasfm;

extern "C" int32_t gasfm_depth_seg_part_rows(int32_t S) { return seg_part_rows(S); }

extern "C" int gasfm_depth_loss_seg_sums(const float* a, const float* b, const int32_t* eoff, int32_t S,
                                         int64_t E_cap, const float* weight, float* part, float* sums,
                                         void* stream) {
  if (int st = check_batch("gasfm_depth_loss_seg_sums", eoff, S, E_cap)) return st;
  GASFM_REQUIRE((E_cap == 0 || (a && b)) && weight && part && sums, "gasfm_depth_loss_seg_sums: null pointer");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(depth_seg_sums_kernel, dim3(kSegG, S), dim3(kT), 0, st, a, b, eoff, E_cap, weight, part);
  hipLaunchKernelGGL(seg_total_kernel<2>, dim3(1), dim3(kT), 0, st, part, S, eoff, weight, sums, nullptr);
  return launch_status("gasfm_depth_loss_seg_sums");
}

extern "C" int gasfm_depth_loss_seg_fwd(const float* a, const float* b, const int32_t* eoff, int32_t S,
                                        int64_t E_cap, const float* weight, const float* sums, int32_t l2,
                                        float* part, float* tot, float* loss, void* stream) {
  if (int st = check_batch("gasfm_depth_loss_seg_fwd", eoff, S, E_cap)) return st;
  GASFM_REQUIRE((E_cap == 0 || (a && b)) && weight && sums && part && tot && loss,
                "gasfm_depth_loss_seg_fwd: null pointer");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(depth_seg_fwd_kernel, dim3(kSegG, S), dim3(kT), 0, st, a, b, eoff, E_cap, weight, sums, l2, part);
  hipLaunchKernelGGL(seg_total_kernel<2>, dim3(1), dim3(kT), 0, st, part, S, eoff, weight, tot, loss);
  return launch_status("gasfm_depth_loss_seg_fwd");
}

extern "C" int gasfm_depth_loss_seg_bwd(const float* a, const float* b, const int32_t* eoff, int32_t S,
                                        int64_t E_cap, const float* weight, const float* sums, const float* tot,
                                        int32_t l2, const float* dloss, float* da, void* stream) {
  if (int st = check_batch("gasfm_depth_loss_seg_bwd", eoff, S, E_cap)) return st;
  GASFM_REQUIRE((E_cap == 0 || (a && b && da)) && weight && sums && tot && dloss,
                "gasfm_depth_loss_seg_bwd: null pointer");
  hipLaunchKernelGGL(depth_seg_bwd_kernel, dim3(kSegG, S), dim3(kT), 0, reinterpret_cast<hipStream_t>(stream), a, b,
                     eoff, E_cap, weight, sums, tot, l2, dloss, da);
  return launch_status("gasfm_depth_loss_seg_bwd");
}

extern "C" int gasfm_depth_scales_seg(const float* dp, const float* dg, const int32_t* eoff, int32_t S,
                                      int64_t E_cap, double* ws, float* scales, void* stream) {
  if (int st = check_batch("gasfm_depth_scales_seg", eoff, S, E_cap)) return st;
  GASFM_REQUIRE((E_cap == 0 || (dp && dg)) && ws && scales, "gasfm_depth_scales_seg: null pointer");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(depth_seg_scale_sums_kernel, dim3(kSegG, S), dim3(kT), 0, st, dp, dg, eoff, E_cap, ws);
  hipLaunchKernelGGL(depth_seg_scales_kernel, dim3(1), dim3(kT), 0, st, ws, S, eoff, scales);
  return launch_status("gasfm_depth_scales_seg");
}

extern "C" int gasfm_backproj_2view_seg(const int32_t* cam, const int32_t* pt, const float* xy, const float* d,
                                        const float* scales, const int32_t* src, const int32_t* eoff, int32_t S,
                                        int64_t E_cap, const float* camtab, int32_t m, float* err, float* rdepth,
                                        float* part, float* tot, void* stream) {
  if (int st = check_batch("gasfm_backproj_2view_seg", eoff, S, E_cap)) return st;
  GASFM_REQUIRE(m >= 0 && scales && part && tot && (E_cap == 0 || (cam && xy && d && src && camtab && m > 0)),
                "gasfm_backproj_2view_seg: null pointer (E_cap=%lld m=%d)", (long long)E_cap, m);
  GASFM_REQUIRE(aligned8(xy) && aligned16(camtab),
                "gasfm_backproj_2view_seg: xy must be 8-byte, camtab 16-byte aligned");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(backproj_seg_kernel, dim3(kSegG, S), dim3(kT), 0, st, cam, pt, xy, d, scales, src, eoff, E_cap,
                     camtab, m, err, rdepth, part);
  hipLaunchKernelGGL(seg_total_kernel<2>, dim3(1), dim3(kT), 0, st, part, S, eoff, nullptr, tot, nullptr);
  return launch_status("gasfm_backproj_2view_seg");
}

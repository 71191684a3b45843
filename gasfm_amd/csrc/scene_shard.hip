// A rank's point shard of a device scene, cut and re-indexed on the device, gfx950.
//
// distributed.shard_scene does this on the host per training sample (numpy selection by point range,
// SceneData.from_sparse, gasfm_build_csr): dist_train.shard_device_scene copies every edge to the host
// and the shard back.  Here the scene's device arrays stay where they are:
//
//   shard_bounds      distributed.partition_points: contiguous point ranges with ~equal edge counts,
//                     one binary search over the point CSR per rank boundary
//   shard_cam_range   edges are cam-major with points ascending inside a camera, so a rank's edges of
//                     camera c are ONE run [lo_c, lo_c + count_c) of the camera's segment: two lower-bound
//                     searches per camera (one thread each); the local cam_ptr is the exclusive scan of
//                     the counts (gasfm_scan_i32)
//   shard_stats       the few scalars the host needs to size the outputs and the plans (one workgroup)
//   shard_emit        local edge j of camera c is global edge lo_c + j - lcam_ptr[c]: the local indices
//                     and bit copies of up to three per-edge [E x 2] fp32 arrays
//   shard_point_csr   the local point CSR from the global one: a point's slots keep their (camera
//                     ascending) order, which is the stable order gasfm_build_csr gives the local edge
//                     list, so perm / pos are equal to the host's element for element
//
// Integer and copy kernels: no float arithmetic, no atomics, no LDS beyond the stats reduction; every
// output is a function of the inputs alone (two runs are bitwise equal).  HBM-bound and small (a
// 118 k-edge scene moves ~5 MB); the launch shapes follow outliers.hip.
#include <hip/hip_runtime.h>

#include "common.hpp"

namespace gasfm {
namespace {

constexpr int kMinViewsPerPoint = 2;  // code/utils/constants.py:2
constexpr int kMinPointsPerView = 8;  // code/utils/constants.py:6
constexpr int kStatsThreads = 1024;

// smallest i in [0, len) with a[i] >= key, len when there is none
template <typename T>
__device__ __forceinline__ int lower_bound(const T* __restrict__ a, int len, int64_t key) {
  int lo = 0, hi = len;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (int64_t(a[mid]) < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// bounds[r] = smallest i with pt_ptr[i] * world >= E * r (r = 1 .. world-1), bounds[0] = 0,
// bounds[world] = n.  pt_ptr is partition_points' csum, and the 64-bit integer comparison equals its
// float one, searchsorted(csum, E * r / world, "left"), for every E * world < 2^53: an integer csum[i]
// below the exact quotient is at least 1 / world below it, which the double nearest to the quotient
// cannot swallow while the quotient is below 2^53 / world.
__global__ __launch_bounds__(256) void shard_bounds_kernel(const int* __restrict__ pt_ptr, int n, int world,
                                                           int* __restrict__ bounds) {
  const int64_t E = pt_ptr[n];
  for (int r = blockIdx.x * 256 + threadIdx.x; r <= world; r += gridDim.x * 256) {
    int b = r == 0 ? 0 : n;
    if (r > 0 && r < world) {
      const int64_t key = E * r;
      int lo = 0, hi = n;  // pt_ptr[n] * world = E * world >= key: the answer is in [0, n]
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (int64_t(pt_ptr[mid]) * world < key) lo = mid + 1; else hi = mid;
      }
      b = lo;
    }
    bounds[r] = b;
  }
}

// one thread per camera c: its run of edges with points in [p0, p1)
template <typename I>
__global__ __launch_bounds__(256) void shard_cam_range_kernel(const int* __restrict__ cam_ptr, const I* __restrict__ pt,
                                                              int m, const int* __restrict__ bounds, int rank,
                                                              int* __restrict__ lo, int* __restrict__ count,
                                                              int64_t* __restrict__ pts_per_cam,
                                                              uint8_t* __restrict__ valid_view) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= m) return;
  const int p0 = bounds[rank], p1 = bounds[rank + 1];
  const int b = cam_ptr[c], e = cam_ptr[c + 1];
  const int l = b + lower_bound(pt + b, e - b, p0);
  const int k = lower_bound(pt + l, e - l, p1);
  lo[c] = l;
  count[c] = k;
  pts_per_cam[c] = k;
  valid_view[c] = uint8_t(e - b >= kMinPointsPerView);  // a global property: replicated on every rank
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = min(v, __shfl_xor(v, o));
  return v;
}

// One workgroup.  out[0..8] = p0, p1, E_loc, then (count, first invalid index relative to the range's
// start, the range's length when all are valid) of: the valid views of [0, m), of the own camera rows
// [c0, c1), and the valid points of [p0, p1).  The valid ids are arange(count) iff first invalid >= count.
__global__ __launch_bounds__(kStatsThreads) void shard_stats_kernel(const int* __restrict__ cam_ptr, int m,
                                                                    const int* __restrict__ pt_ptr,
                                                                    const int* __restrict__ bounds, int rank, int c0,
                                                                    int c1, int64_t* __restrict__ out) {
  __shared__ int red[6][kStatsThreads / 64];
  const int t = threadIdx.x;
  const int p0 = bounds[rank], p1 = bounds[rank + 1];
  int v[6] = {0, m, 0, c1 - c0, 0, p1 - p0};
  for (int c = t; c < m; c += kStatsThreads) {
    const bool ok = cam_ptr[c + 1] - cam_ptr[c] >= kMinPointsPerView;
    const bool own = c >= c0 && c < c1;
    v[0] += ok;
    if (!ok) v[1] = min(v[1], c);
    v[2] += ok && own;
    if (!ok && own) v[3] = min(v[3], c - c0);
  }
  for (int p = p0 + t; p < p1; p += kStatsThreads) {
    const bool ok = pt_ptr[p + 1] - pt_ptr[p] >= kMinViewsPerPoint;
    v[4] += ok;
    if (!ok) v[5] = min(v[5], p - p0);
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const int w = i & 1 ? wave_min(v[i]) : wave_sum(v[i]);
    if ((t & 63) == 0) red[i][t >> 6] = w;
  }
  __syncthreads();
  if (t == 0) {
    out[0] = p0;
    out[1] = p1;
    out[2] = pt_ptr[p1] - pt_ptr[p0];
    for (int i = 0; i < 6; ++i) {
      int a = red[i][0];
      for (int w = 1; w < kStatsThreads / 64; ++w) a = i & 1 ? min(a, red[i][w]) : a + red[i][w];
      out[3 + i] = a;
    }
  }
}

// grid-stride over the local edges
template <typename I>
__global__ __launch_bounds__(256) void shard_emit_kernel(
    const int* __restrict__ lcam_ptr, const int* __restrict__ lo, int m, const I* __restrict__ pt, int64_t E_loc, int p0,
    const float2* __restrict__ src0, const float2* __restrict__ src1, const float2* __restrict__ src2,
    int64_t* __restrict__ sel, int64_t* __restrict__ indices, int* __restrict__ cam32, int* __restrict__ pt32,
    float2* __restrict__ dst0, float2* __restrict__ dst1, float2* __restrict__ dst2) {
  for (int64_t j = int64_t(blockIdx.x) * 256 + threadIdx.x; j < E_loc; j += int64_t(gridDim.x) * 256) {
    // the camera whose local segment holds j: the last c with lcam_ptr[c] <= j (cameras without a
    // local edge share their successor's start; lcam_ptr[m] = E_loc > j ends the search)
    int a = 0, b = m;
    while (a < b) {
      const int mid = (a + b) >> 1;
      if (lcam_ptr[mid + 1] <= j) a = mid + 1; else b = mid;
    }
    const int c = a < m ? a : m - 1;  // a < m whenever lcam_ptr[m] = E_loc
    const int64_t g = int64_t(lo[c]) + (j - lcam_ptr[c]);
    const int q = int(int64_t(pt[g]) - p0);
    sel[j] = g;
    indices[j] = c;
    indices[E_loc + j] = q;
    cam32[j] = c;
    pt32[j] = q;
    if (src0) dst0[j] = src0[g];
    if (src1) dst1[j] = src1[g];
    if (src2) dst2[j] = src2[g];
  }
}

// grid-stride over max(n_loc + 1, E_loc): the point-sized outputs and the local perm / pos
template <typename I>
__global__ __launch_bounds__(256) void shard_point_csr_kernel(
    const int* __restrict__ pt_ptr, const int* __restrict__ perm, const I* __restrict__ cam,
    const int* __restrict__ lcam_ptr, const int* __restrict__ lo, int p0, int n_loc, int64_t E_loc, int64_t total,
    int* __restrict__ lpt_ptr, int64_t* __restrict__ cam_per_pts, uint8_t* __restrict__ valid_pt,
    int* __restrict__ lperm, int* __restrict__ lpos) {
  const int base = pt_ptr[p0];
  for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < total; i += int64_t(gridDim.x) * 256) {
    if (i <= n_loc) {
      const int here = pt_ptr[p0 + i];
      lpt_ptr[i] = here - base;
      if (i < n_loc) {
        const int d = pt_ptr[p0 + i + 1] - here;
        cam_per_pts[i] = d;
        valid_pt[i] = uint8_t(d >= kMinViewsPerPoint);
      }
    }
    if (i < E_loc) {
      // the edge at point-order position base + i; inside a point the global CSR lists cameras
      // ascending, as the stable grouping of the (cam-major) local edge list does
      const int64_t g = perm ? perm[base + i] : base + i;
      const int c = int(cam[g]);
      const int64_t id = lcam_ptr[c] + (g - lo[c]);
      if (id >= 0 && id < E_loc) {  // holds for a consistent scene; keeps a broken one inside the buffers
        lperm[i] = int(id);
        lpos[id] = int(i);
      }
    }
  }
}

}  // namespace
}  // namespace gasfm

using namespace gasfm;

extern "C" int gasfm_scene_shard_bounds(const int32_t* pt_ptr, int32_t n, int32_t world, int32_t* bounds,
                                        void* stream) {
  GASFM_REQUIRE(n >= 0 && world >= 1, "gasfm_scene_shard_bounds: n=%d world=%d", n, world);
  GASFM_REQUIRE(pt_ptr && bounds, "gasfm_scene_shard_bounds: null pointer");
  hipLaunchKernelGGL(shard_bounds_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, pt_ptr, n, world, bounds);
  return launch_status("gasfm_scene_shard_bounds");
}

extern "C" int gasfm_scene_shard_cam_range(const int32_t* cam_ptr, const void* pt, int32_t pt_is64, int32_t m,
                                           const int32_t* bounds, int32_t rank, int32_t* lo, int32_t* count,
                                           int64_t* pts_per_cam, uint8_t* valid_view, void* stream) {
  GASFM_REQUIRE(m >= 0 && rank >= 0, "gasfm_scene_shard_cam_range: m=%d rank=%d", m, rank);
  if (m == 0) return GASFM_OK;
  GASFM_REQUIRE(cam_ptr && pt && bounds && lo && count && pts_per_cam && valid_view,
                "gasfm_scene_shard_cam_range: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((m + 255) / 256);
  if (pt_is64)
    hipLaunchKernelGGL(shard_cam_range_kernel<int64_t>, grid, dim3(256), 0, st, cam_ptr,
                       static_cast<const int64_t*>(pt), m, bounds, rank, lo, count, pts_per_cam, valid_view);
  else
    hipLaunchKernelGGL(shard_cam_range_kernel<int32_t>, grid, dim3(256), 0, st, cam_ptr,
                       static_cast<const int32_t*>(pt), m, bounds, rank, lo, count, pts_per_cam, valid_view);
  return launch_status("gasfm_scene_shard_cam_range");
}

extern "C" int gasfm_scene_shard_stats(const int32_t* cam_ptr, int32_t m, const int32_t* pt_ptr, int32_t n,
                                       const int32_t* bounds, int32_t rank, int32_t c0, int32_t c1, int64_t* out,
                                       void* stream) {
  GASFM_REQUIRE(m >= 0 && n >= 0 && rank >= 0 && 0 <= c0 && c0 <= c1 && c1 <= m,
                "gasfm_scene_shard_stats: m=%d n=%d rank=%d cameras [%d, %d)", m, n, rank, c0, c1);
  GASFM_REQUIRE(cam_ptr && pt_ptr && bounds && out, "gasfm_scene_shard_stats: null pointer");
  hipLaunchKernelGGL(shard_stats_kernel, dim3(1), dim3(kStatsThreads), 0, (hipStream_t)stream, cam_ptr, m, pt_ptr,
                     bounds, rank, c0, c1, out);
  return launch_status("gasfm_scene_shard_stats");
}

extern "C" int gasfm_scene_shard_emit(const int32_t* lcam_ptr, const int32_t* lo, int32_t m, const void* pt,
                                      int32_t pt_is64, int64_t E_loc, int32_t p0, const float* src0,
                                      const float* src1, const float* src2, int64_t* sel, int64_t* indices,
                                      int32_t* cam32, int32_t* pt32, float* dst0, float* dst1, float* dst2,
                                      void* stream) {
  GASFM_REQUIRE(m >= 0 && E_loc >= 0 && E_loc < (int64_t(1) << 31) && p0 >= 0,
                "gasfm_scene_shard_emit: m=%d E_loc=%lld p0=%d", m, (long long)E_loc, p0);
  if (E_loc == 0) return GASFM_OK;
  GASFM_REQUIRE(m > 0 && lcam_ptr && lo && pt && sel && indices && cam32 && pt32,
                "gasfm_scene_shard_emit: null pointer");
  GASFM_REQUIRE((!src0 || dst0) && (!src1 || dst1) && (!src2 || dst2),
                "gasfm_scene_shard_emit: a source array without its destination");
  for (const float* p : {src0, src1, src2, (const float*)dst0, (const float*)dst1, (const float*)dst2})
    GASFM_REQUIRE((reinterpret_cast<uintptr_t>(p) & 7u) == 0, "gasfm_scene_shard_emit: rows not 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  auto f2 = [](const float* p) { return reinterpret_cast<const float2*>(p); };
  auto d2 = [](float* p) { return reinterpret_cast<float2*>(p); };
  if (pt_is64) {
    const int grid = resident_grid(reinterpret_cast<const void*>(shard_emit_kernel<int64_t>), 256, 0, E_loc, 256 * 4);
    hipLaunchKernelGGL(shard_emit_kernel<int64_t>, dim3(grid), dim3(256), 0, st, lcam_ptr, lo, m,
                       static_cast<const int64_t*>(pt), E_loc, p0, f2(src0), f2(src1), f2(src2), sel, indices, cam32,
                       pt32, d2(dst0), d2(dst1), d2(dst2));
  } else {
    const int grid = resident_grid(reinterpret_cast<const void*>(shard_emit_kernel<int32_t>), 256, 0, E_loc, 256 * 4);
    hipLaunchKernelGGL(shard_emit_kernel<int32_t>, dim3(grid), dim3(256), 0, st, lcam_ptr, lo, m,
                       static_cast<const int32_t*>(pt), E_loc, p0, f2(src0), f2(src1), f2(src2), sel, indices, cam32,
                       pt32, d2(dst0), d2(dst1), d2(dst2));
  }
  return launch_status("gasfm_scene_shard_emit");
}

extern "C" int gasfm_scene_shard_point_csr(const int32_t* pt_ptr, const int32_t* perm, const void* cam,
                                           int32_t cam_is64, const int32_t* lcam_ptr, const int32_t* lo, int32_t p0,
                                           int32_t n_loc, int64_t E_loc, int32_t* lpt_ptr, int64_t* cam_per_pts,
                                           uint8_t* valid_pt, int32_t* lperm, int32_t* lpos, void* stream) {
  GASFM_REQUIRE(p0 >= 0 && n_loc >= 0 && E_loc >= 0 && E_loc < (int64_t(1) << 31),
                "gasfm_scene_shard_point_csr: p0=%d n_loc=%d E_loc=%lld", p0, n_loc, (long long)E_loc);
  GASFM_REQUIRE(pt_ptr && lpt_ptr && (n_loc == 0 || (cam_per_pts && valid_pt)) &&
                    (E_loc == 0 || (cam && lcam_ptr && lo && lperm && lpos)),
                "gasfm_scene_shard_point_csr: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const int64_t total = E_loc > n_loc + 1 ? E_loc : int64_t(n_loc) + 1;
  if (cam_is64) {
    const int grid =
        resident_grid(reinterpret_cast<const void*>(shard_point_csr_kernel<int64_t>), 256, 0, total, 256 * 4);
    hipLaunchKernelGGL(shard_point_csr_kernel<int64_t>, dim3(grid), dim3(256), 0, st, pt_ptr, perm,
                       static_cast<const int64_t*>(cam), lcam_ptr, lo, p0, n_loc, E_loc, total, lpt_ptr, cam_per_pts,
                       valid_pt, lperm, lpos);
  } else {
    const int grid =
        resident_grid(reinterpret_cast<const void*>(shard_point_csr_kernel<int32_t>), 256, 0, total, 256 * 4);
    hipLaunchKernelGGL(shard_point_csr_kernel<int32_t>, dim3(grid), dim3(256), 0, st, pt_ptr, perm,
                       static_cast<const int32_t*>(cam), lcam_ptr, lo, p0, n_loc, E_loc, total, lpt_ptr, cam_per_pts,
                       valid_pt, lperm, lpos);
  }
  return launch_status("gasfm_scene_shard_point_csr");
}

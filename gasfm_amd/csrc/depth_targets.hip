// Per-edge depth targets of a scene on the device, gfx950: build, sample, augment.
//
// The reference keeps the targets of the depth head as a dense [m, n] float matrix
// (datasets/SceneData.py:57-134: depths = (K_inv @ y @ X)[:, 2, :]), indexes it when a scene is
// sampled (:318-350) and rescales all of it in the rotational homography augmentation (:431-434);
// its loss reads the visible entries only.  Here a scene carries d [E] float32 in its camera-major
// edge order (the order of data.x.indices, which DirectDepthLoss takes) and no dense array exists:
//
//   depth_targets   d[e] = a[cam[e]] . X[pt[e]]: a [m, 4] = the third rows of Ns[c] @ y[c] (m-sized,
//                   from the host), X [n, 4] the triangulated points with last coordinate 1; counts
//                   the edges whose depth is not finite or not > 0 (the reference's two asserts)
//   depth_gather    sampling: sampled edge (c', p') is the parent's edge (view_idx[c'], keep[p']); its
//                   position in the parent's camera row [cam_ptr[c], cam_ptr[c + 1]) is a binary
//                   search over the row's ascending point ids; counts the edges it did not find
//   depth_rescale   augmentation: d'[e] = d[e] / z_old * z_new, z_old = (Ns[c] @ (u, v, 1))[2],
//                   z_new = (R[c] @ (Ns[c] @ (u, v, 1)))[2], (u, v) the OLD pixel measurement of the
//                   edge read from the un-augmented dense M; fp32, divide then multiply
//
// One thread per edge in a grid-stride loop, consecutive threads on consecutive edges (cam / pt /
// value reads and the store coalesce; inside a camera the points ascend, so the X and M reads are
// near-ordered gathers).  No LDS, no atomics: a count is summed over each wave with lane shuffles,
// lane 0 writes the wave's partial (a vector store) and a one-wave kernel adds the partials in slot
// order.  Every output is a function of the inputs alone (two runs are bitwise equal).  An index
// outside its array is never followed: the edge counts as bad / missing and its output is NaN.
#include <hip/hip_runtime.h>

#include <cmath>

#include "common.hpp"

namespace gasfm {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxBlocks = 1024;  // 4 resident workgroups on each of the 256 CUs

inline int depth_blocks(int64_t E) {
  const int64_t want = (E + kThreads - 1) / kThreads;
  return int(want < 1 ? 1 : (want > kMaxBlocks ? kMaxBlocks : want));
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// every wave's count into its own slot; all 64 lanes reach this (no early exit in the callers)
__device__ __forceinline__ void write_wave_count(int count, int32_t* __restrict__ part) {
  const int total = wave_sum(count);
  if ((threadIdx.x & 63) == 0) part[blockIdx.x * kWaves + (threadIdx.x >> 6)] = total;
}

// One wave: out[0] = part[0] + ... + part[slots - 1] (integers: any order gives the same sum).
__global__ __launch_bounds__(64) void count_sum_kernel(const int32_t* __restrict__ part, int slots,
                                                       int32_t* __restrict__ out) {
  int v = 0;
  for (int i = threadIdx.x; i < slots; i += 64) v += part[i];
  v = wave_sum(v);
  if (threadIdx.x == 0) out[0] = v;
}

template <typename I>
__global__ __launch_bounds__(kThreads) void depth_targets_kernel(const float4* __restrict__ a, int m,
                                                                 const float4* __restrict__ X, int n,
                                                                 const I* __restrict__ cam, const I* __restrict__ pt,
                                                                 int64_t E, float* __restrict__ d,
                                                                 int32_t* __restrict__ part) {
  int bad = 0;
  for (int64_t e = int64_t(blockIdx.x) * kThreads + threadIdx.x; e < E; e += int64_t(gridDim.x) * kThreads) {
    const int64_t c = cam[e], p = pt[e];
    float v = NAN;
    if (c >= 0 && c < m && p >= 0 && p < n) {
      const float4 r = a[c], x = X[p];
      v = r.x * x.x + r.y * x.y + r.z * x.z + r.w * x.w;
    }
    d[e] = v;
    bad += !(isfinite(v) && v > 0.0f);
  }
  write_wave_count(bad, part);
}

template <typename I, typename J>
__global__ __launch_bounds__(kThreads) void depth_gather_kernel(
    const int32_t* __restrict__ pcam_ptr, const J* __restrict__ ppt, const float* __restrict__ pd, int mp, int64_t Ep,
    const int64_t* __restrict__ view_idx, const int64_t* __restrict__ keep, int ms, int ns, const I* __restrict__ cam,
    const I* __restrict__ pt, int64_t E, float* __restrict__ d, int32_t* __restrict__ part) {
  int missing = 0;
  for (int64_t e = int64_t(blockIdx.x) * kThreads + threadIdx.x; e < E; e += int64_t(gridDim.x) * kThreads) {
    const int64_t c = cam[e], p = pt[e];
    float v = NAN;
    bool found = false;
    if (c >= 0 && c < ms && p >= 0 && p < ns) {
      const int64_t pc = view_idx[c], key = keep[p];
      if (pc >= 0 && pc < mp) {
        int64_t lo = pcam_ptr[pc], hi = pcam_ptr[pc + 1];
        lo = lo < 0 ? 0 : lo;
        hi = hi > Ep ? Ep : hi;  // a broken cam_ptr stays inside ppt / pd
        const int64_t end = hi;
        while (lo < hi) {  // the first position of the row with a point id >= key
          const int64_t mid = (lo + hi) >> 1;
          if (int64_t(ppt[mid]) < key) lo = mid + 1; else hi = mid;
        }
        if (lo < end && int64_t(ppt[lo]) == key) {
          v = pd[lo];
          found = true;
        }
      }
    }
    d[e] = v;
    missing += !found;
  }
  write_wave_count(missing, part);
}

template <typename I>
__global__ __launch_bounds__(kThreads) void depth_rescale_kernel(const float* __restrict__ d,
                                                                 const I* __restrict__ cam, const I* __restrict__ pt,
                                                                 int64_t E, const float* __restrict__ M, int64_t ldM,
                                                                 int m, int n, const float* __restrict__ Ns,
                                                                 const float* __restrict__ R, float* __restrict__ out) {
  for (int64_t e = int64_t(blockIdx.x) * kThreads + threadIdx.x; e < E; e += int64_t(gridDim.x) * kThreads) {
    const int64_t c = cam[e], p = pt[e];
    float v = NAN;
    if (c >= 0 && c < m && p >= 0 && p < n) {
      const float u = M[2 * c * ldM + p], w = M[(2 * c + 1) * ldM + p];
      const float* __restrict__ N = Ns + 9 * c;
      const float* __restrict__ r = R + 9 * c;
      // Ns[c] @ (u, v, 1), then the third row of R[c] on it
      const float q0 = N[0] * u + N[1] * w + N[2];
      const float q1 = N[3] * u + N[4] * w + N[5];
      const float q2 = N[6] * u + N[7] * w + N[8];
      const float z_new = r[6] * q0 + r[7] * q1 + r[8] * q2;
      v = d[e] / q2 * z_new;
    }
    out[e] = v;
  }
}

int sum_counts(const int32_t* part, int slots, int32_t* out, hipStream_t st, const char* where) {
  hipLaunchKernelGGL(count_sum_kernel, dim3(1), dim3(64), 0, st, part, slots, out);
  return launch_status(where);
}

}  // namespace
}  // namespace gasfm

using namespace gasfm;

extern "C" int64_t gasfm_depth_part_slots(int64_t E) { return E <= 0 ? 0 : int64_t(depth_blocks(E)) * kWaves; }

extern "C" int gasfm_depth_targets(const float* a, int32_t m, const float* X, int32_t n, const void* cam,
                                   const void* pt, int32_t idx_is64, int64_t E, float* d, int32_t* part,
                                   int32_t* bad, void* stream) {
  GASFM_REQUIRE(m >= 0 && n >= 0 && E >= 0, "gasfm_depth_targets: m=%d n=%d E=%lld", m, n, (long long)E);
  if (E == 0) return GASFM_OK;
  GASFM_REQUIRE(a && X && cam && pt && d && part && bad, "gasfm_depth_targets: null pointer");
  GASFM_REQUIRE(aligned16(a) && aligned16(X), "gasfm_depth_targets: a / X rows not 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int grid = depth_blocks(E);
  const float4* a4 = reinterpret_cast<const float4*>(a);
  const float4* X4 = reinterpret_cast<const float4*>(X);
  if (idx_is64)
    hipLaunchKernelGGL(depth_targets_kernel<int64_t>, dim3(grid), dim3(kThreads), 0, st, a4, m, X4, n,
                       static_cast<const int64_t*>(cam), static_cast<const int64_t*>(pt), E, d, part);
  else
    hipLaunchKernelGGL(depth_targets_kernel<int32_t>, dim3(grid), dim3(kThreads), 0, st, a4, m, X4, n,
                       static_cast<const int32_t*>(cam), static_cast<const int32_t*>(pt), E, d, part);
  const int status = launch_status("gasfm_depth_targets");
  if (status != GASFM_OK) return status;
  return sum_counts(part, grid * kWaves, bad, st, "gasfm_depth_targets (count)");
}

extern "C" int gasfm_depth_gather(const int32_t* pcam_ptr, const void* ppt, int32_t ppt_is64, const float* pd,
                                  int32_t mp, int64_t Ep, const int64_t* view_idx, const int64_t* keep, int32_t ms,
                                  int32_t ns, const void* cam, const void* pt, int32_t idx_is64, int64_t E, float* d,
                                  int32_t* part, int32_t* missing, void* stream) {
  GASFM_REQUIRE(mp >= 0 && Ep >= 0 && ms >= 0 && ns >= 0 && E >= 0, "gasfm_depth_gather: mp=%d Ep=%lld ms=%d ns=%d E=%lld",
                mp, (long long)Ep, ms, ns, (long long)E);
  if (E == 0) return GASFM_OK;
  GASFM_REQUIRE(pcam_ptr && view_idx && keep && cam && pt && d && part && missing && (Ep == 0 || (ppt && pd)),
                "gasfm_depth_gather: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const int grid = depth_blocks(E);
#define GASFM_GATHER(I, J)                                                                                          \
  hipLaunchKernelGGL((depth_gather_kernel<I, J>), dim3(grid), dim3(kThreads), 0, st, pcam_ptr,                     \
                     static_cast<const J*>(ppt), pd, mp, Ep, view_idx, keep, ms, ns, static_cast<const I*>(cam), \
                     static_cast<const I*>(pt), E, d, part)
  if (idx_is64 && ppt_is64) GASFM_GATHER(int64_t, int64_t);
  else if (idx_is64) GASFM_GATHER(int64_t, int32_t);
  else if (ppt_is64) GASFM_GATHER(int32_t, int64_t);
  else GASFM_GATHER(int32_t, int32_t);
#undef GASFM_GATHER
  const int status = launch_status("gasfm_depth_gather");
  if (status != GASFM_OK) return status;
  return sum_counts(part, grid * kWaves, missing, st, "gasfm_depth_gather (count)");
}

extern "C" int gasfm_depth_rescale(const float* d, const void* cam, const void* pt, int32_t idx_is64, int64_t E,
                                   const float* M, int64_t ldM, int32_t m, int32_t n, const float* Ns, const float* R,
                                   float* out, void* stream) {
  GASFM_REQUIRE(m >= 0 && n >= 0 && E >= 0 && ldM >= n, "gasfm_depth_rescale: m=%d n=%d E=%lld ldM=%lld", m, n,
                (long long)E, (long long)ldM);
  if (E == 0) return GASFM_OK;
  GASFM_REQUIRE(d && cam && pt && M && Ns && R && out, "gasfm_depth_rescale: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const int grid = depth_blocks(E);
  if (idx_is64)
    hipLaunchKernelGGL(depth_rescale_kernel<int64_t>, dim3(grid), dim3(kThreads), 0, st, d,
                       static_cast<const int64_t*>(cam), static_cast<const int64_t*>(pt), E, M, ldM, m, n, Ns, R, out);
  else
    hipLaunchKernelGGL(depth_rescale_kernel<int32_t>, dim3(grid), dim3(kThreads), 0, st, d,
                       static_cast<const int32_t*>(cam), static_cast<const int32_t*>(pt), E, M, ldM, m, n, Ns, R, out);
  return launch_status("gasfm_depth_rescale");
}

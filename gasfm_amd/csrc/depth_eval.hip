// Depth-head evaluation over the visibility edges (code/evaluation.py:33-72, 241-301), gfx950.
//
// The reference backprojects every pixel of every view with its predicted depth, hands each
// backprojected point to another view of the same track and reprojects it there
// (geo_utils.reprojection_error_backproj_random_view_pairs, geo_utils.py:393-464): several dense
// [m, n, 3] fp64 arrays on the host.  Here only the E observed (camera, point) pairs are touched:
//   track_cycle_kernel      a wave per point: src[e'] = the edge of the same track one rank below e'
//                           in the order of (random key, edge id), cyclically -- the reference's
//                           shuffle + cyclic 1-shift of each track
//   backproj_2view_kernel   a thread per destination edge: gather the partner edge, backproject with
//                           its camera, project with the destination's; per-edge error / depth
//                           (optional) and per-workgroup (sum, count) of the non-NaN errors
//   depth_sum / depth_norm  the mean depths (determine_depth_scale) and the sum / min / max of the
//                           mean-normalised depths and of their L1 distance
// No atomics; every reduction runs in a fixed order (fp64 for the depth sums), nothing is read back
// on the host and every size follows from (E, m, n): two runs give the same bits and each entry can
// be captured.
#include "../../include/gasfm_depth_eval.h"
#include "depth_edge.hpp"
#include "edge_loss.hpp"

namespace gasfm {
namespace {

constexpr int kW = kT / 64;

// ---------------------------------------------------------------- track pairing
__device__ __forceinline__ int64_t rank_word(int32_t key, int32_t e) {
  return (int64_t(key) << 32) | int64_t(uint32_t(e));  // signed order = (key, edge id)
}

__device__ __forceinline__ int64_t lane_word(int64_t v, int t) {
  const int lo = __builtin_amdgcn_readlane(int(uint32_t(uint64_t(v))), t);
  const int hi = __builtin_amdgcn_readlane(int(uint32_t(uint64_t(v) >> 32)), t);
  return int64_t((uint64_t(uint32_t(hi)) << 32) | uint64_t(uint32_t(lo)));
}

// (rank word, usable) of CSR position i0 + at + lane of a track of L positions
struct TrackLane {
  int64_t word;
  int32_t edge;
  bool ok;
};

__device__ __forceinline__ TrackLane track_lane(const int32_t* __restrict__ perm, const int32_t* __restrict__ key,
                                                int64_t E, int64_t i0, int64_t at, int64_t L, int lane) {
  TrackLane r{0, -1, false};
  if (at + lane < L) {
    const int64_t i = i0 + at + lane;
    r.edge = perm ? perm[i] : int32_t(i);
    r.ok = uint32_t(r.edge) < uint64_t(E);
    if (r.ok) r.word = rank_word(key[r.edge], r.edge);
  }
  return r;
}

// One wave per point.  Every lane owns the positions lane, lane + 64, ... of the track and looks for
// the predecessor of each of them in the (key, edge id) order: the largest word below its own, or the
// largest of the track when it is the smallest itself.  The track passes by in chunks of 64 held one
// per lane and read lane by lane (v_readlane: no LDS).  L^2 / 64 steps per wave for any L.
__global__ __launch_bounds__(kT) void track_cycle_kernel(const int32_t* __restrict__ pt_ptr,
                                                         const int32_t* __restrict__ perm,
                                                         const int32_t* __restrict__ key, int64_t E, int64_t n,
                                                         int32_t* __restrict__ src) {
  const int64_t p = int64_t(blockIdx.x) * kW + int64_t(threadIdx.x >> 6);
  if (p >= n) return;  // whole waves leave together
  const int lane = threadIdx.x & 63;
  int64_t i0 = pt_ptr[p], i1 = pt_ptr[p + 1];
  i0 = i0 < 0 ? 0 : i0;
  i1 = i1 > E ? E : i1;
  const int64_t L = i1 - i0;
  if (L <= 0) return;
  if (L == 1) {
    const TrackLane me = track_lane(perm, key, E, i0, 0, L, lane);
    if (me.ok) src[me.edge] = -1;
    return;
  }
  for (int64_t a = 0; a < L; a += 64) {
    const TrackLane me = track_lane(perm, key, E, i0, a, L, lane);
    bool below = false, any = false;
    int64_t best_below = 0, best = 0;
    for (int64_t b = 0; b < L; b += 64) {
      const TrackLane it = (b == a) ? me : track_lane(perm, key, E, i0, b, L, lane);
      const uint64_t usable = __ballot(it.ok);
      const int cnt = int(L - b < 64 ? L - b : 64);
      for (int t = 0; t < cnt; ++t) {
        if (!((usable >> t) & 1)) continue;  // uniform
        const int64_t w = lane_word(it.word, t);
        if (!any || w > best) best = w;
        any = true;
        if (w < me.word && (!below || w > best_below)) {
          best_below = w;
          below = true;
        }
      }
    }
    if (me.ok) src[me.edge] = int32_t(uint32_t(uint64_t(below ? best_below : best)));
  }
}

// bad[0] = the number of tracks of length 1, by one workgroup in a fixed order
__global__ __launch_bounds__(kT) void track_single_kernel(const int32_t* __restrict__ pt_ptr, int64_t n,
                                                          int32_t* __restrict__ bad) {
  __shared__ int32_t sh[kT];
  int32_t c = 0;
  for (int64_t p = threadIdx.x; p < n; p += kT) c += (pt_ptr[p + 1] - pt_ptr[p]) == 1;
  sh[threadIdx.x] = c;
  __syncthreads();
  for (int s = kT / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) bad[0] = sh[0];
}

// ---------------------------------------------------------------- 2-view error
// CamRow, load_row and the per-edge body backproj_edge: depth_edge.hpp (shared with depth_batch.hip)
__global__ __launch_bounds__(kT) void backproj_2view_kernel(const int32_t* __restrict__ cam,
                                                            const int32_t* __restrict__ pt,
                                                            const float* __restrict__ xy,
                                                            const float* __restrict__ d,
                                                            const float* __restrict__ scale,
                                                            const int32_t* __restrict__ src, int64_t E,
                                                            const float* __restrict__ tab, int32_t m,
                                                            float* __restrict__ err, float* __restrict__ rdepth,
                                                            float* __restrict__ part) {
  __shared__ float sh[kW * 2];
  float acc[2] = {0.f, 0.f};
  const float s = E > 0 ? scale[0] : 0.f;
  for (int64_t e2 = int64_t(blockIdx.x) * kT + threadIdx.x; e2 < E; e2 += int64_t(gridDim.x) * kT) {
    float r, z;
    backproj_edge(cam, pt, xy, d, s, src, E, tab, m, e2, r, z);
    if (err) err[e2] = r;
    if (rdepth) rdepth[e2] = z;
    const bool ok = !isnan(r);
    acc[0] += ok ? r : 0.f;
    acc[1] += ok ? 1.f : 0.f;
  }
  const float t = block_sums(acc, sh);
  if (threadIdx.x < 2) part[2 * int64_t(blockIdx.x) + threadIdx.x] = t;
}

// ---------------------------------------------------------------- depth scales and statistics
__device__ __forceinline__ double nan_min(double a, double b) { return (a < b || a != a) ? a : b; }
__device__ __forceinline__ double nan_max(double a, double b) { return (a > b || a != a) ? a : b; }

constexpr int kStat = 7;  // sum, min, max of the predictions; of the targets; sum of |difference|

struct Stat {
  double v[kStat];
};

__device__ __forceinline__ Stat stat_identity() {
  const double inf = double(INFINITY);
  return Stat{{0.0, inf, -inf, 0.0, inf, -inf, 0.0}};
}

__device__ __forceinline__ Stat stat_merge(const Stat& a, const Stat& b) {
  return Stat{{a.v[0] + b.v[0], nan_min(a.v[1], b.v[1]), nan_max(a.v[2], b.v[2]), a.v[3] + b.v[3],
               nan_min(a.v[4], b.v[4]), nan_max(a.v[5], b.v[5]), a.v[6] + b.v[6]}};
}

// block_tree, Sum2 and sum2_merge: depth_edge.hpp

// sums[row] = fp64 (sum dp, sum dg) of workgroup row's grid-stride slice
__global__ __launch_bounds__(kT) void depth_sum_kernel(const float* __restrict__ dp, const float* __restrict__ dg,
                                                       int64_t E, double* __restrict__ sums) {
  __shared__ Sum2 sh[kT];
  Sum2 a{0.0, 0.0};
  for (int64_t e = int64_t(blockIdx.x) * kT + threadIdx.x; e < E; e += int64_t(gridDim.x) * kT) {
    a.a += double(dp[e]);
    if (dg) a.b += double(dg[e]);
  }
  a = block_tree(a, sh, sum2_merge);
  if (threadIdx.x == 0) {
    sums[2 * int64_t(blockIdx.x)] = a.a;
    sums[2 * int64_t(blockIdx.x) + 1] = a.b;
  }
}

// scales = float(sum / E) of the partial rows in order; rows = 0 (no edges) or no targets: NaN
__global__ __launch_bounds__(kT) void depth_scale_kernel(const double* __restrict__ sums, int rows, int64_t E,
                                                         int has_dg, float* __restrict__ scales) {
  __shared__ Sum2 sh[kT];
  Sum2 a{0.0, 0.0};
  for (int r = threadIdx.x; r < rows; r += kT) a = sum2_merge(a, Sum2{sums[2 * r], sums[2 * r + 1]});
  a = block_tree(a, sh, sum2_merge);
  if (threadIdx.x == 0) {
    const float nan = __int_as_float(0x7fc00000);
    scales[0] = rows > 0 ? float(a.a / double(E)) : nan;
    scales[1] = rows > 0 && has_dg ? float(a.b / double(E)) : nan;
  }
}

__global__ __launch_bounds__(kT) void depth_norm_kernel(const float* __restrict__ dp, const float* __restrict__ dg,
                                                        int64_t E, const float* __restrict__ scales,
                                                        double* __restrict__ part) {
  __shared__ Stat sh[kT];
  Stat a = stat_identity();
  const float sp = scales[0], sg = scales[1];
  for (int64_t e = int64_t(blockIdx.x) * kT + threadIdx.x; e < E; e += int64_t(gridDim.x) * kT) {
    const float x = dp[e] / sp;
    Stat one = stat_identity();
    one.v[0] = one.v[1] = one.v[2] = double(x);
    if (dg) {
      const float y = dg[e] / sg;
      one.v[3] = one.v[4] = one.v[5] = double(y);
      one.v[6] = double(fabsf(x - y));
    }
    a = stat_merge(a, one);
  }
  a = block_tree(a, sh, stat_merge);
  if (threadIdx.x == 0)
#pragma unroll
    for (int i = 0; i < kStat; ++i) part[kStat * int64_t(blockIdx.x) + i] = a.v[i];
}

__global__ __launch_bounds__(kT) void depth_norm_finish_kernel(const double* __restrict__ part, int rows, int has_dg,
                                                               double* __restrict__ stats) {
  __shared__ Stat sh[kT];
  Stat a = stat_identity();
  for (int r = threadIdx.x; r < rows; r += kT) {
    Stat one;
#pragma unroll
    for (int i = 0; i < kStat; ++i) one.v[i] = part[kStat * int64_t(r) + i];
    a = stat_merge(a, one);
  }
  a = block_tree(a, sh, stat_merge);
  if (threadIdx.x == 0) {
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
#pragma unroll
    for (int i = 0; i < kStat; ++i) stats[i] = (rows > 0 && (i < 3 || has_dg)) ? a.v[i] : nan;
  }
}

}  // namespace
}  // namespace gasfm

using namespace gasfm;

extern "C" int gasfm_track_cycle(const int32_t* pt_ptr, const int32_t* perm, const int32_t* key, int64_t E, int64_t n,
                                 int32_t* src, int32_t* bad, void* stream) {
  GASFM_REQUIRE(E >= 0 && n >= 0 && E <= INT32_MAX && n <= INT32_MAX, "gasfm_track_cycle: E=%lld n=%lld", (long long)E,
                (long long)n);
  GASFM_REQUIRE(bad && (n == 0 || pt_ptr) && (E == 0 || (key && src)), "gasfm_track_cycle: null pointer");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (E > 0 && n > 0)
    hipLaunchKernelGGL(track_cycle_kernel, dim3(unsigned((n + kW - 1) / kW)), dim3(kT), 0, st, pt_ptr, perm, key, E, n,
                       src);
  hipLaunchKernelGGL(track_single_kernel, dim3(1), dim3(kT), 0, st, pt_ptr, n, bad);
  return launch_status("gasfm_track_cycle");
}

extern "C" int32_t gasfm_backproj_2view_part_rows(int64_t E) { return part_rows(E); }

extern "C" int gasfm_backproj_2view(const int32_t* cam, const int32_t* pt, const float* xy, const float* d,
                                    const float* scale, const int32_t* src, int64_t E, const float* camtab, int32_t m,
                                    float* err, float* rdepth, float* part, void* stream) {
  GASFM_REQUIRE(E >= 0 && m >= 0 && E <= INT32_MAX, "gasfm_backproj_2view: E=%lld m=%d", (long long)E, m);
  GASFM_REQUIRE(part && (E == 0 || (cam && xy && d && scale && src && camtab && m > 0)),
                "gasfm_backproj_2view: null pointer (E=%lld m=%d)", (long long)E, m);
  GASFM_REQUIRE(aligned8(xy) && aligned16(camtab), "gasfm_backproj_2view: xy must be 8-byte, camtab 16-byte aligned");
  hipLaunchKernelGGL(backproj_2view_kernel, dim3(part_rows(E)), dim3(kT), 0, reinterpret_cast<hipStream_t>(stream), cam,
                     pt, xy, d, scale, src, E, camtab, m, err, rdepth, part);
  return launch_status("gasfm_backproj_2view");
}

extern "C" int64_t gasfm_depth_norm_stats_ws_doubles(int64_t E) { return (2 + kStat) * int64_t(part_rows(E)); }

extern "C" int gasfm_depth_norm_stats(const float* dp, const float* dg, int64_t E, double* ws, float* scales,
                                      double* stats, void* stream) {
  GASFM_REQUIRE(E >= 0 && E <= INT32_MAX, "gasfm_depth_norm_stats: E=%lld", (long long)E);
  GASFM_REQUIRE(scales && (E == 0 || (dp && ws)), "gasfm_depth_norm_stats: null pointer (E=%lld)", (long long)E);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int rows = E > 0 ? part_rows(E) : 0;
  const int has_dg = dg != nullptr;
  double* part = ws ? ws + 2 * int64_t(rows) : nullptr;
  if (rows > 0) hipLaunchKernelGGL(depth_sum_kernel, dim3(rows), dim3(kT), 0, st, dp, dg, E, ws);
  hipLaunchKernelGGL(depth_scale_kernel, dim3(1), dim3(kT), 0, st, ws, rows, E, has_dg, scales);
  if (stats) {
    if (rows > 0) hipLaunchKernelGGL(depth_norm_kernel, dim3(rows), dim3(kT), 0, st, dp, dg, E, scales, part);
    hipLaunchKernelGGL(depth_norm_finish_kernel, dim3(1), dim3(kT), 0, st, part, rows, has_dg, stats);
  }
  return launch_status("gasfm_depth_norm_stats");
}

// Depth statistics of compute_errors (code/evaluation.py:351-363) over the visibility edges, gfx950.
//
// The reference forms pts2D = Ps @ pflat(pts3D) ([m, 3, n]: 600M elements at config 4), compares
// its z row with loss.infinity_pts_margin and reduces the dense masks.  Here only the E observed
// (camera, point) pairs are projected, as in esfm_loss.hip:
//   depth_e = Ps_pix[c, 2, :] . (pts3D[:, p] / pts3D[3, p])          (pflat first, like the reference)
//   neg_e   = !(depth_e >= margin)                                   (a NaN depth is negative)
// Three launches, ordered by the stream (no hand-off between workgroups inside a launch):
//   depth_edge_kernel    grid-stride over the edges: depth[e] (optional) and one partial row per
//                        workgroup (#neg as int64, sum in fp64, min, max)
//   depth_seg_any_kernel cam_neg[c] (a wave per camera over its contiguous edges) and pt_neg[p]
//                        (a thread per point through the point CSR / perm); the depth is
//                        recomputed by the same expression, so the flags agree with the edge pass
//   depth_finish_kernel  one workgroup: partial rows and non-empty segments in a fixed order
// Counts stay integers until the last store; the sum is fp64 over fp32 depths; min / max and the
// sum propagate NaN (ndarray.min / max / mean).  No float atomics, no atomics at all: two runs on
// the same input give the same bits.
#include <hip/hip_runtime.h>

#include "common.hpp"

namespace gasfm {
namespace {

constexpr int kT = 256;
constexpr int kW = kT / 64;
constexpr int kMaxRows = 1024;

__device__ __forceinline__ float edge_depth(const float* __restrict__ P, const float* __restrict__ X, int64_t n,
                                            int c, int p) {
  const float* pc = P + int64_t(c) * 12 + 8;
  const float w = X[3 * n + p];
  const float x0 = X[p] / w, x1 = X[n + p] / w, x2 = X[2 * n + p] / w, x3 = w / w;
  return fmaf(pc[0], x0, fmaf(pc[1], x1, fmaf(pc[2], x2, pc[3] * x3)));
}

// min / max that keep a NaN operand (fminf / fmaxf drop it)
__device__ __forceinline__ double nan_min(double a, double b) { return (a < b || a != a) ? a : b; }
__device__ __forceinline__ double nan_max(double a, double b) { return (a > b || a != a) ? a : b; }

struct Acc {
  long long neg;
  double sum, lo, hi;
};

__device__ __forceinline__ Acc acc_identity() { return Acc{0, 0.0, double(INFINITY), -double(INFINITY)}; }

__device__ __forceinline__ Acc acc_merge(const Acc& a, const Acc& b) {
  return Acc{a.neg + b.neg, a.sum + b.sum, nan_min(a.lo, b.lo), nan_max(a.hi, b.hi)};
}

// workgroup reduction in a fixed order (tree over the thread index); the result is in thread 0
__device__ __forceinline__ Acc block_reduce(Acc v, Acc* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int s = kT / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) sh[threadIdx.x] = acc_merge(sh[threadIdx.x], sh[threadIdx.x + s]);
    __syncthreads();
  }
  return sh[0];
}

// part row b = (neg count [int64 bits], sum, min, max) of workgroup b's grid-stride slice
__global__ __launch_bounds__(kT) void depth_edge_kernel(const int32_t* __restrict__ cam,
                                                        const int32_t* __restrict__ pt, int64_t E,
                                                        const float* __restrict__ P, const float* __restrict__ X,
                                                        int64_t n, float margin, float* __restrict__ depth,
                                                        double* __restrict__ part) {
  __shared__ Acc sh[kT];
  Acc a = acc_identity();
  for (int64_t e = int64_t(blockIdx.x) * kT + threadIdx.x; e < E; e += int64_t(gridDim.x) * kT) {
    const float d = edge_depth(P, X, n, cam[e], pt[e]);
    if (depth) depth[e] = d;
    a.neg += !(d >= margin);
    a.sum += double(d);
    a.lo = nan_min(double(d), a.lo);
    a.hi = nan_max(double(d), a.hi);
  }
  a = block_reduce(a, sh);
  if (threadIdx.x == 0) {
    double* row = part + 4 * int64_t(blockIdx.x);
    row[0] = __longlong_as_double(a.neg);
    row[1] = a.sum;
    row[2] = a.lo;
    row[3] = a.hi;
  }
}

// blocks [0, cam_blocks): a wave per camera; the rest: a thread per point
__global__ __launch_bounds__(kT) void depth_seg_any_kernel(const int32_t* __restrict__ cam_ptr, int32_t m,
                                                           const int32_t* __restrict__ pt_ptr,
                                                           const int32_t* __restrict__ perm,
                                                           const int32_t* __restrict__ cam,
                                                           const int32_t* __restrict__ pt,
                                                           const float* __restrict__ P, const float* __restrict__ X,
                                                           int64_t n, float margin, int cam_blocks,
                                                           int32_t* __restrict__ cam_neg,
                                                           int32_t* __restrict__ pt_neg) {
  if (int(blockIdx.x) < cam_blocks) {
    const int c = int(blockIdx.x) * kW + int(threadIdx.x >> 6);
    if (c >= m) return;  // whole waves leave together
    const int lane = threadIdx.x & 63;
    bool neg = false;
    for (int64_t e = int64_t(cam_ptr[c]) + lane, e1 = cam_ptr[c + 1]; e < e1; e += 64)
      neg |= !(edge_depth(P, X, n, c, pt[e]) >= margin);
    const bool any = __ballot(neg) != 0;
    if (lane == 0) cam_neg[c] = any ? 1 : 0;
    return;
  }
  const int64_t p = int64_t(int(blockIdx.x) - cam_blocks) * kT + threadIdx.x;
  if (p >= n) return;
  bool neg = false;
  for (int i = pt_ptr[p], i1 = pt_ptr[p + 1]; i < i1; ++i) {
    const int e = perm ? perm[i] : i;
    neg |= !(edge_depth(P, X, n, cam[e], int(p)) >= margin);
  }
  pt_neg[p] = neg ? 1 : 0;
}

// stats = (#neg edges, #cameras with an edge, #points with an edge, sum, min, max)
__global__ __launch_bounds__(kT) void depth_finish_kernel(const double* __restrict__ part, int rows,
                                                          const int32_t* __restrict__ cam_ptr, int32_t m,
                                                          const int32_t* __restrict__ pt_ptr, int64_t n,
                                                          double* __restrict__ stats) {
  __shared__ Acc sh[kT];
  Acc a = acc_identity();
  for (int r = threadIdx.x; r < rows; r += kT) {
    const double* row = part + 4 * int64_t(r);
    a = acc_merge(a, Acc{__double_as_longlong(row[0]), row[1], row[2], row[3]});
  }
  a = block_reduce(a, sh);
  __syncthreads();
  // the two segment counts ride through the same reduction (neg: cameras, sum unused)
  Acc s = acc_identity();
  for (int c = threadIdx.x; c < m; c += kT) s.neg += cam_ptr[c + 1] > cam_ptr[c];
  s = block_reduce(s, sh);
  const long long n_cam = s.neg;
  __syncthreads();
  s = acc_identity();
  for (int64_t p = threadIdx.x; p < n; p += kT) s.neg += pt_ptr[p + 1] > pt_ptr[p];
  s = block_reduce(s, sh);
  if (threadIdx.x == 0) {
    stats[0] = double(a.neg);
    stats[1] = double(n_cam);
    stats[2] = double(s.neg);
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    stats[3] = rows > 0 ? a.sum : nan;  // no edges: ndarray.mean / min / max of an empty selection
    stats[4] = rows > 0 ? a.lo : nan;
    stats[5] = rows > 0 ? a.hi : nan;
  }
}

int part_rows(int64_t E) {
  const int64_t b = (E + kT - 1) / kT;
  return int(b < 1 ? 1 : (b > kMaxRows ? kMaxRows : b));
}

}  // namespace
}  // namespace gasfm

using namespace gasfm;

extern "C" int64_t gasfm_depth_stats_ws_doubles(int64_t E) { return 4 * int64_t(part_rows(E)); }

extern "C" int gasfm_depth_stats(const int32_t* cam, const int32_t* pt, int64_t E, const int32_t* cam_ptr, int32_t m,
                                 const int32_t* pt_ptr, const int32_t* perm, int64_t n, const float* P,
                                 const float* pts3D, float margin, float* depth, int32_t* cam_neg, int32_t* pt_neg,
                                 double* ws, double* stats, void* stream) {
  GASFM_REQUIRE(E >= 0 && m >= 0 && n >= 0 && E <= INT32_MAX && n <= INT32_MAX,
                "gasfm_depth_stats: E=%lld m=%d n=%lld", (long long)E, m, (long long)n);
  GASFM_REQUIRE(stats && (m == 0 || cam_neg) && (n == 0 || pt_neg), "gasfm_depth_stats: null output");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (E == 0) {
    // nothing to project: zero flags, zero counts and NaN sum / min / max (the finish kernel with no
    // partial rows and no segments); no kernel is handed a null input
    int s = GASFM_OK;
    if (m > 0) s = hip_status(hipMemsetAsync(cam_neg, 0, sizeof(int32_t) * size_t(m), st), "gasfm_depth_stats");
    if (s == GASFM_OK && n > 0)
      s = hip_status(hipMemsetAsync(pt_neg, 0, sizeof(int32_t) * size_t(n), st), "gasfm_depth_stats");
    if (s != GASFM_OK) return s;
    hipLaunchKernelGGL(depth_finish_kernel, dim3(1), dim3(kT), 0, st, nullptr, 0, nullptr, 0, nullptr, int64_t(0),
                       stats);
    return launch_status("gasfm_depth_stats");
  }
  GASFM_REQUIRE(m > 0 && n > 0 && cam && pt && cam_ptr && pt_ptr && P && pts3D && ws,
                "gasfm_depth_stats: null pointer (E=%lld m=%d n=%lld)", (long long)E, m, (long long)n);
  const int rows = part_rows(E);
  hipLaunchKernelGGL(depth_edge_kernel, dim3(rows), dim3(kT), 0, st, cam, pt, E, P, pts3D, n, margin, depth, ws);
  const int cam_blocks = (m + kW - 1) / kW;
  const int pt_blocks = int((n + kT - 1) / kT);
  hipLaunchKernelGGL(depth_seg_any_kernel, dim3(cam_blocks + pt_blocks), dim3(kT), 0, st, cam_ptr, m, pt_ptr, perm,
                     cam, pt, P, pts3D, n, margin, cam_blocks, cam_neg, pt_neg);
  hipLaunchKernelGGL(depth_finish_kernel, dim3(1), dim3(kT), 0, st, ws, rows, cam_ptr, m, pt_ptr, n, stats);
  return launch_status("gasfm_depth_stats");
}

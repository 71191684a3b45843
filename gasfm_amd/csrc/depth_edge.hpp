// Per-edge pieces of the depth-head evaluation shared by the single-scene kernels (depth_eval.hip) and
// the union-batch ones (depth_batch.hip): the 2-view error of one destination edge, and the fp64
// fixed-order workgroup sum of the depth scales.
#pragma once
#include "../../include/gasfm_depth_eval.h"
#include "edge_loss.hpp"

namespace gasfm {

// camera row: [R | t] at 0, K^-1 at 12, K at 21 (GASFM_CAMTAB_FLOATS floats, 128 bytes)
struct CamRow {
  float4 q[8];
  __device__ __forceinline__ float at(int i) const { return reinterpret_cast<const float*>(q)[i]; }
};

// float4s [first, first + count) of camera c's row
template <int kFirst, int kCount>
__device__ __forceinline__ void load_row(const float* __restrict__ tab, int c, CamRow& r) {
  const float4* row = reinterpret_cast<const float4*>(tab + int64_t(c) * GASFM_CAMTAB_FLOATS);
#pragma unroll
  for (int i = kFirst; i < kFirst + kCount; ++i) r.q[i] = row[i];
}

// The 2-view error r and the reprojected depth z of destination edge e2 with the depths rescaled by s:
// NaN where src[e2] is outside [0, E), a camera is outside [0, m) or (pt given) the source belongs to
// another track.
__device__ __forceinline__ void backproj_edge(const int32_t* __restrict__ cam, const int32_t* __restrict__ pt,
                                              const float* __restrict__ xy, const float* __restrict__ d, float s,
                                              const int32_t* __restrict__ src, int64_t E,
                                              const float* __restrict__ tab, int32_t m, int64_t e2, float& r,
                                              float& z) {
  const float nan = __int_as_float(0x7fc00000);
  r = nan, z = nan;
  const int32_t e = src[e2], c2 = cam[e2];
  if (uint32_t(e) < uint64_t(E) && uint32_t(c2) < uint32_t(m)) {
    const int32_t c = cam[e];
    if (uint32_t(c) < uint32_t(m) && (!pt || pt[e] == pt[e2])) {
      CamRow A, B;
      load_row<0, 6>(tab, c, A);   // [R | t], K^-1 of the source camera
      load_row<0, 3>(tab, c2, B);  // [R | t], K of the destination camera
      load_row<5, 3>(tab, c2, B);
      const float2 m1 = reinterpret_cast<const float2*>(xy)[e];
      const float2 m2 = reinterpret_cast<const float2*>(xy)[e2];
      float h[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) h[i] = fmaf(A.at(12 + 3 * i), m1.x, fmaf(A.at(13 + 3 * i), m1.y, A.at(14 + 3 * i)));
      const float dd = s * d[e];
      const float l[3] = {dd * (h[0] / h[2]) - A.at(3), dd * (h[1] / h[2]) - A.at(7), dd - A.at(11)};
      float X[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) X[k] = fmaf(A.at(k), l[0], fmaf(A.at(4 + k), l[1], A.at(8 + k) * l[2]));
      float q[3], y[3];
#pragma unroll
      for (int i = 0; i < 3; ++i)
        q[i] = fmaf(B.at(4 * i), X[0], fmaf(B.at(4 * i + 1), X[1], fmaf(B.at(4 * i + 2), X[2], B.at(4 * i + 3))));
#pragma unroll
      for (int i = 0; i < 3; ++i)
        y[i] = fmaf(B.at(21 + 3 * i), q[0], fmaf(B.at(22 + 3 * i), q[1], B.at(23 + 3 * i) * q[2]));
      const float u = m2.x - y[0] / y[2], v = m2.y - y[1] / y[2];
      r = sqrtf(fmaf(u, u, v * v));
      z = q[2];
    }
  }
}

// tree over the thread index: a fixed order; the result is in every thread
template <class T, class Merge>
__device__ __forceinline__ T block_tree(T v, T* sh, Merge merge) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int s = kT / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) sh[threadIdx.x] = merge(sh[threadIdx.x], sh[threadIdx.x + s]);
    __syncthreads();
  }
  return sh[0];
}

struct Sum2 {
  double a, b;
};

__device__ __forceinline__ Sum2 sum2_merge(const Sum2& x, const Sum2& y) { return Sum2{x.a + y.a, x.b + y.b}; }

}  // namespace gasfm

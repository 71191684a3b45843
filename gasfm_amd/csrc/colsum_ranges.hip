// Ordered, weighted column sums over contiguous row ranges, fp64 accumulate, ONE launch:
//   out[s, j] = sum_{r = row_ptr[s]}^{row_ptr[s+1]-1} w[r] * A[r, j]      (w null: plain sums)
// The per-scene sums of a union of scenes (gasfm_amd/setofset.py): the ranges are the scenes' camera,
// point or edge rows, so camera ranges are 10-20 rows and edge ranges tens of thousands.
//
// Layout: workgroup (s, chunk) owns range s and a chunk of up to 32 columns.  Its 256 threads are
// G column groups (a float4 each when cols % 4 == 0 and A is 16-byte aligned, else one column) x
// RL = 256 / G row lanes; row lane l sums rows r0 + l, r0 + l + RL, ... in that order (8 independent
// loads in flight, added in row order), then the lanes fold through LDS by halving strides.  The
// order of every addition is a function of (row_ptr, cols) alone: nothing depends on the grid or
// on timing, there are no atomics and no workspace, and an empty range writes zeros.  A range is
// never split across workgroups, only its columns are: cols / 32 workgroups per range, each row
// lane reading one 128-byte line per row.  Within a workgroup a range splits into batches of
// 8 * RL rows (256 rows at 32 float4-read columns) and a row-by-row tail.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.hpp"

namespace gasfm {

constexpr int kRangeBlock = 256;
constexpr int kRangeChunk = 32;   // columns per workgroup
constexpr int kRangeUnroll = 8;   // rows in flight per row lane

template <bool kVec, bool kW>
__global__ __launch_bounds__(kRangeBlock) void colsum_ranges_kernel(const float* __restrict__ A, int64_t ld, int cols,
                                                                    const int32_t* __restrict__ row_ptr,
                                                                    const double* __restrict__ w,
                                                                    double* __restrict__ out) {
  // [RL, ccols] lane sums, row-lane major: RL * ccols <= 256 * 4 (kVec) or 256
  __shared__ double sh[kRangeBlock * 4];
  const int s = blockIdx.x, cbase = blockIdx.y * kRangeChunk, t = threadIdx.x;
  const int ccols = (cols - cbase) < kRangeChunk ? (cols - cbase) : kRangeChunk;
  const int64_t r0 = row_ptr[s], r1 = row_ptr[s + 1];
  const int G = kVec ? ccols / 4 : ccols;
  const int RL = kRangeBlock / G;
  const int cg = t % G, rl = t / G;
  if (rl < RL) {
    const float* __restrict__ Ab = A + cbase + (kVec ? 4 * cg : cg);
    int64_t r = r0 + rl;
    if constexpr (kVec) {
      double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
      for (; r + int64_t(kRangeUnroll - 1) * RL < r1; r += int64_t(kRangeUnroll) * RL) {
        float4 v[kRangeUnroll];
        double ww[kRangeUnroll];
#pragma unroll
        for (int u = 0; u < kRangeUnroll; ++u) {
          v[u] = *reinterpret_cast<const float4*>(Ab + (r + int64_t(u) * RL) * ld);
          ww[u] = kW ? w[r + int64_t(u) * RL] : 1.0;
        }
#pragma unroll
        for (int u = 0; u < kRangeUnroll; ++u) {
          a0 += ww[u] * double(v[u].x);
          a1 += ww[u] * double(v[u].y);
          a2 += ww[u] * double(v[u].z);
          a3 += ww[u] * double(v[u].w);
        }
      }
      for (; r < r1; r += RL) {
        const float4 v = *reinterpret_cast<const float4*>(Ab + r * ld);
        const double ww = kW ? w[r] : 1.0;
        a0 += ww * double(v.x);
        a1 += ww * double(v.y);
        a2 += ww * double(v.z);
        a3 += ww * double(v.w);
      }
      double* q = sh + rl * ccols + 4 * cg;
      q[0] = a0;
      q[1] = a1;
      q[2] = a2;
      q[3] = a3;
    } else {
      double a = 0.0;
      for (; r + int64_t(kRangeUnroll - 1) * RL < r1; r += int64_t(kRangeUnroll) * RL) {
        float v[kRangeUnroll];
        double ww[kRangeUnroll];
#pragma unroll
        for (int u = 0; u < kRangeUnroll; ++u) {
          v[u] = Ab[(r + int64_t(u) * RL) * ld];
          ww[u] = kW ? w[r + int64_t(u) * RL] : 1.0;
        }
#pragma unroll
        for (int u = 0; u < kRangeUnroll; ++u) a += ww[u] * double(v[u]);
      }
      for (; r < r1; r += RL) a += (kW ? w[r] : 1.0) * double(Ab[r * ld]);
      sh[rl * ccols + cg] = a;
    }
  }
  __syncthreads();
  // fold the RL row lanes: rows [h, 2h) onto [0, h), h = P / 2, P / 4, ..., 1 (P: RL rounded up to a
  // power of two; rows past RL do not exist)
  int P = 1;
  while (P < RL) P <<= 1;
  const int live = RL * ccols;
  for (int h = P >> 1; h >= 1; h >>= 1) {
    const int n = h * ccols;
    for (int i = t; i < n; i += kRangeBlock)
      if (i + n < live) sh[i] += sh[i + n];
    __syncthreads();
  }
  if (t < ccols) out[int64_t(s) * cols + cbase + t] = sh[t];
}

}  // namespace gasfm

using namespace gasfm;

extern "C" int gasfm_colsum_ranges(const float* A, int64_t ld, int32_t cols, const int32_t* row_ptr,
                                   int32_t n_ranges, const double* w, double* out, void* stream) {
  GASFM_REQUIRE(cols >= 1 && ld >= cols && n_ranges >= 0, "gasfm_colsum_ranges: cols=%d ld=%lld n_ranges=%d", cols,
                (long long)ld, n_ranges);
  if (n_ranges == 0) return GASFM_OK;
  GASFM_REQUIRE(row_ptr && out, "gasfm_colsum_ranges: null pointer");
  const int nchunk = (cols + kRangeChunk - 1) / kRangeChunk;
  GASFM_REQUIRE(nchunk <= 65535, "gasfm_colsum_ranges: cols=%d exceeds %d", cols, 65535 * kRangeChunk);
  const bool vec = (cols & 3) == 0 && (ld & 3) == 0 && aligned16(A);
  const dim3 grid(n_ranges, nchunk), block(kRangeBlock);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (vec && w)
    hipLaunchKernelGGL((colsum_ranges_kernel<true, true>), grid, block, 0, st, A, ld, cols, row_ptr, w, out);
  else if (vec)
    hipLaunchKernelGGL((colsum_ranges_kernel<true, false>), grid, block, 0, st, A, ld, cols, row_ptr, w, out);
  else if (w)
    hipLaunchKernelGGL((colsum_ranges_kernel<false, true>), grid, block, 0, st, A, ld, cols, row_ptr, w, out);
  else
    hipLaunchKernelGGL((colsum_ranges_kernel<false, false>), grid, block, 0, st, A, ld, cols, row_ptr, w, out);
  return launch_status("gasfm_colsum_ranges");
}

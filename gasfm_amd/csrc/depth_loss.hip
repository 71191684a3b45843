// DirectDepthLoss (code/loss_functions.py:24-66) over the E visibility edges, gfx950.
//
// a = predicted depths (the depth head's value per edge), b = target depths at the same edges:
//   s_a = mean a, s_b = mean b                      (geo_utils.determine_depth_scale)
//   u_e = a_e / s_a - b_e / s_b
//   loss = mean |u_e| (L1)  or  mean u_e^2 (L2)
//   dloss/da_k = (g_k / s_a - (sum_e g_e a_e) / (E s_a^2)) / E,   g = sign(u) (0 at u = 0) or 2u
// Three launches, each scale read from device memory (no host read, no atomics):
//   depth_sums  -> per-workgroup (sum a, sum b)            -> ordered colsum -> sums
//   depth_fwd   -> per-workgroup (sum l_e, sum g_e a_e)    -> ordered colsum -> tot
//   depth_bwd   -> da, elementwise
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "depth_term.hpp"
#include "lanes.hpp"

namespace gasfm {
namespace {

constexpr int kT = 256;

// (sum of v0, sum of v1) over the workgroup, valid in thread 0
__device__ __forceinline__ void block_sum2(float& v0, float& v1, float* sh) {
  v0 = group_sum<64>(v0);
  v1 = group_sum<64>(v1);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    sh[2 * wave] = v0;
    sh[2 * wave + 1] = v1;
  }
  __syncthreads();
  v0 = v1 = 0.f;
  for (int w = 0; w < kT / 64; ++w) {
    v0 += sh[2 * w];
    v1 += sh[2 * w + 1];
  }
}

__global__ __launch_bounds__(kT) void depth_sums_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                        int64_t E, float* __restrict__ part) {
  __shared__ float sh[2 * kT / 64];
  float sa = 0.f, sb = 0.f;
  for (int64_t e = int64_t(blockIdx.x) * kT + threadIdx.x; e < E; e += int64_t(gridDim.x) * kT) {
    sa += a[e];
    sb += b[e];
  }
  block_sum2(sa, sb, sh);
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = sa;
    part[2 * blockIdx.x + 1] = sb;
  }
}

// depth_term (depth_term.hpp): u_e, l_e and g_e of one edge, shared with depth_batch.hip

__global__ __launch_bounds__(kT) void depth_fwd_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                       int64_t E, const float* __restrict__ sums, int l2,
                                                       float* __restrict__ part) {
  __shared__ float sh[2 * kT / 64];
  const float Sa = sums[0], Sb = sums[1], k = float(E) / (Sa * Sb);
  float sl = 0.f, sga = 0.f;
  for (int64_t e = int64_t(blockIdx.x) * kT + threadIdx.x; e < E; e += int64_t(gridDim.x) * kT) {
    float l, g;
    const float ae = a[e];
    depth_term(ae, b[e], Sa, Sb, k, l2, l, g);
    sl += l;
    sga = fmaf(g, ae, sga);
  }
  block_sum2(sl, sga, sh);
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = sl;
    part[2 * blockIdx.x + 1] = sga;
  }
}

__global__ __launch_bounds__(kT) void depth_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                       int64_t E, const float* __restrict__ sums,
                                                       const float* __restrict__ tot, int l2,
                                                       const float* __restrict__ dloss, float* __restrict__ da) {
  const int64_t e = int64_t(blockIdx.x) * kT + threadIdx.x;
  if (e >= E) return;
  const float inv_e = 1.f / float(E);
  const float Sa = sums[0], Sb = sums[1], k = float(E) / (Sa * Sb), inv_sa = float(E) / Sa;
  float l, g;
  depth_term(a[e], b[e], Sa, Sb, k, l2, l, g);
  // d(a_e / s_a)/da_k = delta_ek / s_a - a_e / (E s_a^2)
  da[e] = dloss[0] * inv_e * inv_sa * (g - tot[1] * inv_e * inv_sa);
}

}  // namespace
}  // namespace gasfm

using namespace gasfm;

extern "C" int32_t gasfm_depth_loss_part_rows(int64_t E) {
  const int64_t b = (E + kT - 1) / kT;
  return int32_t(b < 1 ? 1 : (b > 1024 ? 1024 : b));
}

extern "C" int gasfm_depth_loss_sums(const float* a, const float* b, int64_t E, float* part, void* stream) {
  GASFM_REQUIRE(E > 0 && a && b && part, "gasfm_depth_loss_sums: E=%lld or null pointer", (long long)E);
  hipLaunchKernelGGL(depth_sums_kernel, dim3(gasfm_depth_loss_part_rows(E)), dim3(kT), 0,
                     reinterpret_cast<hipStream_t>(stream), a, b, E, part);
  return launch_status("gasfm_depth_loss_sums");
}

extern "C" int gasfm_depth_loss_fwd(const float* a, const float* b, int64_t E, const float* sums, int32_t l2,
                                    float* part, void* stream) {
  GASFM_REQUIRE(E > 0 && a && b && sums && part, "gasfm_depth_loss_fwd: E=%lld or null pointer", (long long)E);
  hipLaunchKernelGGL(depth_fwd_kernel, dim3(gasfm_depth_loss_part_rows(E)), dim3(kT), 0,
                     reinterpret_cast<hipStream_t>(stream), a, b, E, sums, l2, part);
  return launch_status("gasfm_depth_loss_fwd");
}

extern "C" int gasfm_depth_loss_bwd(const float* a, const float* b, int64_t E, const float* sums, const float* tot,
                                    int32_t l2, const float* dloss, float* da, void* stream) {
  GASFM_REQUIRE(E > 0 && a && b && sums && tot && dloss && da, "gasfm_depth_loss_bwd: E=%lld or null pointer",
                (long long)E);
  hipLaunchKernelGGL(depth_bwd_kernel, dim3(unsigned((E + kT - 1) / kT)), dim3(kT), 0,
                     reinterpret_cast<hipStream_t>(stream), a, b, E, sums, tot, l2, dloss, da);
  return launch_status("gasfm_depth_loss_bwd");
}

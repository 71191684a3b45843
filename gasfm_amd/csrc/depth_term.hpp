// The per-edge term of DirectDepthLoss, shared by the single-scene kernels (depth_loss.hip) and the
// union-batch ones (depth_batch.hip): both evaluate the same arithmetic per edge.
#pragma once
#include <hip/hip_runtime.h>

namespace gasfm {

// u_e = a / s_a - b / s_b as (a Sb - b Sa) E / (Sa Sb) with Sa = sum a, Sb = sum b: the two products
// are rounded separately (fma contraction off), so u_e is exactly 0 where a_e / s_a = b_e / s_b holds
// exactly (E = 1; equal depths under equal scales), as the reference's x / x = 1 makes it.
__device__ __forceinline__ void depth_term(float a, float b, float Sa, float Sb, float k, int l2, float& l, float& g) {
#pragma clang fp contract(off)
  const float u = (a * Sb - b * Sa) * k;
  if (l2) {
    l = u * u;
    g = 2.f * u;
  } else {
    l = fabsf(u);
    g = u > 0.f ? 1.f : (u < 0.f ? -1.f : 0.f);  // torch's sign: 0 at 0
  }
}

}  // namespace gasfm

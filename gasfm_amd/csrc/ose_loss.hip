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
// Deterministic: fixed-order sums, no atomics, no host read.  The kernels are edge_loss.hpp's,
// instantiated for the term below.
#include "edge_loss.hpp"

namespace gasfm {
namespace {

struct OseTerm {
  static constexpr int kStats = 1;  // sum of l_e
  static constexpr bool kIsLoss = true, kGradReadsTot = false;
  float w_reg;

  // l_e
  __device__ __forceinline__ float value(const float* __restrict__ P, const float* __restrict__ X, int64_t n, int c,
                                         int p, float mx, float my, float (&stats)[1]) const {
    float y[3], xs[4];
    project(P, X, n, c, p, y, xs);
    const float rx = y[0] - y[2] * mx, ry = y[1] - y[2] * my;
    return stats[0] = sqrtf(rx * rx + ry * ry) + w_reg * expf(-y[2]);
  }

  static __device__ __forceinline__ EdgeScale scales(float up, float ne, const float*, int) {
    return {up / ne, 0.f, 0.f};
  }

  // G_e
  __device__ __forceinline__ void grad(const float (&y)[3], float mx, float my, const EdgeScale& k,
                                       float (&g)[3]) const {
    const float rx = y[0] - y[2] * mx, ry = y[1] - y[2] * my;
    const float nr = sqrtf(rx * rx + ry * ry);
    const float s = nr > 0.f ? k.scale / nr : 0.f;  // d||r||/dr = r / ||r|| (0 at r = 0, as torch)
    g[0] = s * rx;
    g[1] = s * ry;
    g[2] = -s * (rx * mx + ry * my) - k.scale * w_reg * expf(-y[2]);
  }
};

}  // namespace
}  // namespace gasfm

using namespace gasfm;

extern "C" int32_t gasfm_ose_part_rows(int64_t E) { return part_rows(E); }

extern "C" int32_t gasfm_ose_seg_part_rows(int32_t S) { return seg_part_rows(S); }

extern "C" int gasfm_ose_fwd(const int32_t* cam, const int32_t* pt, const float* vals, int64_t E, const float* P,
                             const float* X, int64_t n, float w_reg, float* part, void* stream) {
  return launch_fwd("gasfm_ose_fwd", cam, pt, vals, E, P, X, n, OseTerm{w_reg}, nullptr, part, stream);
}

extern "C" int gasfm_ose_bwd(const int32_t* cptr, int32_t m, const int32_t* pptr, const int32_t* perm,
                             const int32_t* cam, const int32_t* pt, const float* vals, int64_t E, const float* P,
                             const float* X, int64_t n, float w_reg, const float* dloss, float* dP, float* dX,
                             void* stream) {
  return launch_bwd<OseTerm, false>("gasfm_ose_bwd", cptr, m, pptr, perm, cam, pt, vals, E, E, Scenes{}, P, X, n,
                                    OseTerm{w_reg}, dloss, nullptr, dP, dX, stream);
}

extern "C" int gasfm_ose_seg_fwd(const int32_t* cam, const int32_t* pt, const float* vals, const int32_t* eoff,
                                 int32_t S, const float* weight, const float* P, const float* X, int64_t n,
                                 float w_reg, float* part, float* tot, float* loss, void* stream) {
  return launch_seg_fwd("gasfm_ose_seg_fwd", cam, pt, vals, eoff, S, weight, P, X, n, OseTerm{w_reg}, part, tot, loss,
                        stream);
}

extern "C" int gasfm_ose_seg_bwd(const int32_t* cam_ptr, int32_t m, const int32_t* pt_ptr, const int32_t* perm,
                                 const int32_t* cam, const int32_t* pt, const float* vals, const int32_t* eoff,
                                 int32_t S, const int32_t* scene_of_cam, const int32_t* scene_of_pt,
                                 const float* weight, const float* P, const float* X, int64_t n, float w_reg,
                                 const float* dloss, float* dP, float* dX, void* stream) {
  return launch_bwd<OseTerm, true>("gasfm_ose_seg_bwd", cam_ptr, m, pt_ptr, perm, cam, pt, vals, 0, 0,
                                   Scenes{eoff, S, scene_of_cam, scene_of_pt, weight}, P, X, n, OseTerm{w_reg}, dloss,
                                   nullptr, dP, dX, stream);
}

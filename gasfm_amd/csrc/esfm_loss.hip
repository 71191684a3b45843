// ESFMLoss (code/loss_functions.py:85-123) as sparse per-edge kernels, gfx950.
//
// The reference forms the dense projections Ps @ pts3D ([m, 3, n]: 2.4 GB at config 4), masks them
// with the dense valid-observation matrix and averages; its backward goes through a gradient hook
// on the [m, 3, n] tensor.  Here every quantity is per visibility edge e = (c, p) (the same E
// edges the network runs on, values[e] = the normalised measurement = norm_M at (c, p)):
//   y_e   = P_c [X_p; w_p]                                        (3-vector)
//   pos_e = y_z >= margin (hinge) or |y_z| >= margin (no hinge)    (geo_utils.py:721-726)
//   l_e   = pos_e ? || y_xy / y_z - m_e || : (margin - y_z) * hinge_w
//   loss  = sum_e l_e / E
// Backward with the reference's hook (pts_grad_equalization_pre_perspective_divide,
// loss_functions.py:104-113): with G_e = dloss * dl_e/dy_e / E (E = E_norm: the global edge count
// when a point-sharded rank passes its own edges),
//   valid-only:  G'_e = pos_e ? normalize(G_e) / max(1, #pos) : G_e
//   otherwise:   G'_e = normalize(G_e) / E
//   none:        G'_e = G_e
// then dP_c = sum_{e in c} G'_e [X_p; w_p]^T (one workgroup per camera, edges in order) and
// d[X_p; w_p] = sum_{e in p} P_c^T G'_e (one thread per point, through the point CSR).
// Deterministic: fixed-order sums, no atomics.  The kernels are edge_loss.hpp's, instantiated for the
// two terms below: this loss and the reprojection error of the evaluation.
#include "edge_loss.hpp"

namespace gasfm {
namespace {

struct EsfmTerm {
  static constexpr int kStats = 2;  // sum of l_e, count of pos_e
  static constexpr bool kIsLoss = true, kGradReadsTot = true;
  float margin, hinge_w;
  int hinge, equalize, valid_only;

  __device__ __forceinline__ bool positive(float z) const { return hinge ? (z >= margin) : (fabsf(z) >= margin); }

  __device__ __forceinline__ float value(const float* __restrict__ P, const float* __restrict__ X, int64_t n, int c,
                                         int p, float mx, float my, float (&stats)[2]) const {
    float y[3], xs[4];
    project(P, X, n, c, p, y, xs);
    const bool pos = positive(y[2]);
    stats[1] = pos ? 1.f : 0.f;
    if (!pos) return stats[0] = (margin - y[2]) * hinge_w;
    const float u = y[0] / y[2] - mx, v = y[1] / y[2] - my;
    return stats[0] = sqrtf(u * u + v * v);
  }

  // E = E_norm: the global edge count when a point-sharded rank passes its own edges
  static __device__ __forceinline__ EdgeScale scales(float up, float ne, const float* __restrict__ tot, int s) {
    const float inv_e = 1.f / ne;
    return {up * inv_e, 1.f / fmaxf(1.f, tot[2 * s + 1]), inv_e};
  }

  // G'_e (see the header)
  __device__ __forceinline__ void grad(const float (&y)[3], float mx, float my, const EdgeScale& k,
                                       float (&g)[3]) const {
    const bool pos = positive(y[2]);
    float d[3];
    if (pos) {
      const float z = y[2], iz = 1.f / z;
      const float u = y[0] * iz - mx, v = y[1] * iz - my;
      const float err = sqrtf(u * u + v * v);
      const float s = err > 0.f ? k.scale / err : 0.f;  // d||.||/d(u,v) = (u, v)/err (0 at err = 0, as torch)
      d[0] = s * u * iz;
      d[1] = s * v * iz;
      d[2] = -s * (u * y[0] + v * y[1]) * iz * iz;
    } else {
      d[0] = d[1] = 0.f;
      d[2] = -hinge_w * k.scale;
    }
    if (equalize && (pos || !valid_only)) {
      const float nrm = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
      const float f = (valid_only ? k.inv_pos : k.inv_e) / fmaxf(nrm, 1e-12f);  // F.normalize eps
#pragma unroll
      for (int i = 0; i < 3; ++i) d[i] *= f;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) g[i] = d[i];
  }
};

// compute_core_errors' "our_repro" (code/evaluation.py:8-31; geo_utils.py:371-391): per edge
//   X = pts3D[:, p] / pts3D[3, p]   (pflat)      y = Ps_pix[c] X      err = ||xy - y_xy / y_z||
// with Ps_pix = Ns^-1 Ps_norm (pixel-space cameras, caller-supplied) and xy the PIXEL
// measurement of the edge.  The per-edge output is err (NaN included); the sums are (the non-NaN
// errors, their count): np.nanmean's operands.  An inf error (y_z == 0, y_xy != 0) is summed like
// numpy does.  Value only.
// kFusedNorm: how u^2 + v^2 is rounded.  The single-list kernel has always been compiled with u * u
// fused into the sum and the per-scene kernel with both products rounded first (1 ulp of err^2
// apart); each entry point is pinned to its own rounding so that its results do not move with the
// compiler's contraction choices.
template <bool kFusedNorm>
struct ReprojTerm {
  static constexpr int kStats = 2;
  static constexpr bool kIsLoss = false;

  __device__ __forceinline__ float value(const float* __restrict__ P, const float* __restrict__ X, int64_t n, int c,
                                         int p, float mx, float my, float (&stats)[2]) const {
    const float w = X[3 * n + p];
    const float x0 = X[p] / w, x1 = X[n + p] / w, x2 = X[2 * n + p] / w;
    const float* pc = P + int64_t(c) * 12;
    float y[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) y[i] = fmaf(pc[4 * i], x0, fmaf(pc[4 * i + 1], x1, fmaf(pc[4 * i + 2], x2, pc[4 * i + 3])));
    const float u = mx - y[0] / y[2], v = my - y[1] / y[2];
    float r;
    if constexpr (kFusedNorm) {
      r = sqrtf(fmaf(u, u, v * v));
    } else {
#pragma clang fp contract(off)
      r = sqrtf(u * u + v * v);
    }
    const bool ok = !isnan(r);
    stats[0] = ok ? r : 0.f;
    stats[1] = ok ? 1.f : 0.f;
    return r;
  }
};

}  // namespace
}  // namespace gasfm

using namespace gasfm;

extern "C" int32_t gasfm_esfm_part_rows(int64_t E) { return part_rows(E); }

extern "C" int32_t gasfm_esfm_seg_part_rows(int32_t S) { return seg_part_rows(S); }

extern "C" int gasfm_esfm_fwd(const int32_t* cam, const int32_t* pt, const float* vals, int64_t E, const float* P,
                              const float* X, int64_t n, float margin, float hinge_w, int32_t hinge, float* part,
                              void* stream) {
  return launch_fwd("gasfm_esfm_fwd", cam, pt, vals, E, P, X, n, EsfmTerm{margin, hinge_w, hinge, 0, 0}, nullptr, part,
                    stream);
}

extern "C" int gasfm_esfm_bwd(const int32_t* cptr, int32_t m, const int32_t* pptr, const int32_t* perm,
                              const int32_t* cam, const int32_t* pt, const float* vals, int64_t E, int64_t E_norm,
                              const float* P, const float* X, int64_t n, float margin, float hinge_w, int32_t hinge,
                              int32_t equalize, int32_t valid_only, const float* dloss, const float* tot, float* dP,
                              float* dX, void* stream) {
  return launch_bwd<EsfmTerm, false>("gasfm_esfm_bwd", cptr, m, pptr, perm, cam, pt, vals, E, E_norm, Scenes{}, P, X, n,
                                     EsfmTerm{margin, hinge_w, hinge, equalize, valid_only}, dloss, tot, dP, dX,
                                     stream);
}

extern "C" int gasfm_esfm_seg_fwd(const int32_t* cam, const int32_t* pt, const float* vals, const int32_t* eoff,
                                  int32_t S, const float* weight, const float* P, const float* X, int64_t n,
                                  float margin, float hinge_w, int32_t hinge, float* part, float* tot, float* loss,
                                  void* stream) {
  return launch_seg_fwd("gasfm_esfm_seg_fwd", cam, pt, vals, eoff, S, weight, P, X, n,
                        EsfmTerm{margin, hinge_w, hinge, 0, 0}, part, tot, loss, stream);
}

extern "C" int gasfm_esfm_seg_bwd(const int32_t* cam_ptr, int32_t m, const int32_t* pt_ptr, const int32_t* perm,
                                  const int32_t* cam, const int32_t* pt, const float* vals, const int32_t* eoff,
                                  int32_t S, const int32_t* scene_of_cam, const int32_t* scene_of_pt,
                                  const float* weight, const float* P, const float* X, int64_t n, float margin,
                                  float hinge_w, int32_t hinge, int32_t equalize, int32_t valid_only,
                                  const float* dloss, const float* tot, float* dP, float* dX, void* stream) {
  return launch_bwd<EsfmTerm, true>("gasfm_esfm_seg_bwd", cam_ptr, m, pt_ptr, perm, cam, pt, vals, 0, 0,
                                    Scenes{eoff, S, scene_of_cam, scene_of_pt, weight}, P, X, n,
                                    EsfmTerm{margin, hinge_w, hinge, equalize, valid_only}, dloss, tot, dP, dX, stream);
}

extern "C" int gasfm_reproj_error(const int32_t* cam, const int32_t* pt, const float* xy, int64_t E, const float* P,
                                  const float* pts3D, int64_t n, float* err, float* part, void* stream) {
  return launch_fwd<ReprojTerm<true>, true>("gasfm_reproj_error", cam, pt, xy, E, P, pts3D, n, {}, err, part, stream);
}

extern "C" int gasfm_reproj_error_seg(const int32_t* cam, const int32_t* pt, const float* xy, const int32_t* eoff,
                                      int32_t S, const float* P, const float* pts3D, int64_t n, float* part,
                                      float* tot, void* stream) {
  return launch_seg_fwd("gasfm_reproj_error_seg", cam, pt, xy, eoff, S, nullptr, P, pts3D, n, ReprojTerm<false>{}, part,
                        tot, nullptr, stream);
}

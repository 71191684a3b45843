// The per-edge scaffold shared by the losses and metrics over the visibility edges (esfm_loss.hip,
// ose_loss.hip), gfx950.  Every quantity is per edge e = (c, p) with a 2-vector vals[e]:
//   forward   sum over the edges of Term::kStats numbers: per-workgroup partials over a grid-stride
//             slice of one edge list, or kSegG slices per scene of a union batch + seg_total
//   backward  G_e = d(term)/dy_e of y_e = P_c [X_p; w_p], then dP_c = sum_{e in c} G_e [X_p; w_p]^T
//             (one workgroup per camera, edges in order) and d[X_p; w_p] = sum_{e in p} P_c^T G_e
//             (one thread per point, through the point CSR)
// Deterministic: fixed-order sums, no atomics, no host read.
//
// A term is a struct that carries its parameters by value:
//   kStats                     columns summed by the forward
//   kIsLoss                    a mean over E > 0 edges with a weighted batch total; a metric may be
//                              empty and has no batch total
//   value(P, X, n, c, p, mx, my, stats)   fills stats[kStats], returns the per-edge output
//   scales(up, ne, tot, s)     the EdgeScale of scene s of ne edges, up = dloss (* weight[s]), tot =
//                              the forward's [S, kStats] totals (static); kGradReadsTot: it reads tot
//   grad(y, mx, my, k, g)      fills g[3] = G_e from the EdgeScale k
// (a value-only term has no scales / grad).
// A union batch: scene s owns edges [eoff[s], eoff[s+1]), its cameras / points are the ones
// scene_of_cam / scene_of_pt map to s.  The batch loss is sum_s weight[s] * loss_s; a scene of
// weight 0 (padding) contributes nothing, and its cameras' and points' gradients are written as
// zeros without reading its projections.
#pragma once
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "lanes.hpp"

namespace gasfm {

constexpr int kT = 256;
constexpr int kSegG = 32;  // workgroups per scene in the segmented sums

inline int32_t part_rows(int64_t E) {
  const int64_t b = (E + kT - 1) / kT;
  return int32_t(b < 1 ? 1 : (b > 1024 ? 1024 : b));
}

inline int32_t seg_part_rows(int32_t S) { return S * kSegG; }

// scale = dloss (* weight) / E, inv_pos = 1 / max(1, #pos), inv_e = 1 / E
struct EdgeScale {
  float scale, inv_pos, inv_e;
};

// y = P_c [X_p; w_p]; xs = the loaded point
__device__ __forceinline__ void project(const float* __restrict__ P, const float* __restrict__ X, int64_t n, int c,
                                        int64_t p, float (&y)[3], float (&xs)[4]) {
  const float* pc = P + int64_t(c) * 12;
  xs[0] = X[p], xs[1] = X[n + p], xs[2] = X[2 * n + p], xs[3] = X[3 * n + p];
#pragma unroll
  for (int i = 0; i < 3; ++i)
    y[i] = fmaf(pc[4 * i], xs[0], fmaf(pc[4 * i + 1], xs[1], fmaf(pc[4 * i + 2], xs[2], pc[4 * i + 3] * xs[3])));
}

// The sums of v[0..N) over the workgroup: each wave's sums go through LDS (sh [kT / 64 * N], used
// once per kernel) and thread i < N returns column i, summed in wave order.
template <int N>
__device__ __forceinline__ float block_sums(float (&v)[N], float* sh) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = group_sum<64>(v[i]);
  if (lane == 0)
#pragma unroll
    for (int i = 0; i < N; ++i) sh[wave * N + i] = v[i];
  __syncthreads();
  float s = 0.f;
  if (threadIdx.x < N)
    for (int w = 0; w < kT / 64; ++w) s += sh[w * N + threadIdx.x];
  return s;
}

// part[row] = the kStats sums over edges e0 + threadIdx.x, + stride, ... < e1; edge_out[e]
// (kEdgeOut, optional) = the term's per-edge output
template <class Term, bool kEdgeOut>
__device__ __forceinline__ void fwd_slice(const int32_t* __restrict__ cam, const int32_t* __restrict__ pt,
                                          const float* __restrict__ vals, int64_t e0, int64_t e1, int64_t stride,
                                          const float* __restrict__ P, const float* __restrict__ X, int64_t n,
                                          const Term& term, float* __restrict__ edge_out, float* __restrict__ part,
                                          int64_t row) {
  __shared__ float sh[kT / 64 * Term::kStats];
  float acc[Term::kStats];
#pragma unroll
  for (int i = 0; i < Term::kStats; ++i) acc[i] = 0.f;
  for (int64_t e = e0 + threadIdx.x; e < e1; e += stride) {
    const float2 m = reinterpret_cast<const float2*>(vals)[e];
    float st[Term::kStats];
    const float v = term.value(P, X, n, cam[e], pt[e], m.x, m.y, st);
    if constexpr (kEdgeOut) {
      if (edge_out) edge_out[e] = v;
    }
#pragma unroll
    for (int i = 0; i < Term::kStats; ++i) acc[i] += st[i];
  }
  const float s = block_sums(acc, sh);
  if (threadIdx.x < Term::kStats) part[Term::kStats * row + threadIdx.x] = s;
}

// one edge list: workgroup b's grid-stride slice
template <class Term, bool kEdgeOut>
__global__ __launch_bounds__(kT) void edge_fwd_kernel(const int32_t* __restrict__ cam, const int32_t* __restrict__ pt,
                                                      const float* __restrict__ vals, int64_t E,
                                                      const float* __restrict__ P, const float* __restrict__ X,
                                                      int64_t n, Term term, float* __restrict__ edge_out,
                                                      float* __restrict__ part) {
  fwd_slice<Term, kEdgeOut>(cam, pt, vals, int64_t(blockIdx.x) * kT, E, int64_t(gridDim.x) * kT, P, X, n, term,
                            edge_out, part, blockIdx.x);
}

// a union batch: part[s * kSegG + g] over scene s = blockIdx.y's edges, slice g = blockIdx.x
template <class Term>
__global__ __launch_bounds__(kT) void edge_fwd_seg_kernel(const int32_t* __restrict__ cam,
                                                          const int32_t* __restrict__ pt,
                                                          const float* __restrict__ vals,
                                                          const int32_t* __restrict__ eoff,
                                                          const float* __restrict__ P, const float* __restrict__ X,
                                                          int64_t n, Term term, float* __restrict__ part) {
  const int s = blockIdx.y;
  fwd_slice<Term, false>(cam, pt, vals, eoff[s] + int64_t(blockIdx.x) * kT, eoff[s + 1], int64_t(kSegG) * kT, P, X, n,
                         term, nullptr, part, int64_t(s) * kSegG + blockIdx.x);
}

// tot[s] = ordered sums of scene s's kSegG partials; loss (optional) = sum over the scenes of
// weight nonzero of weight[s] * tot[s][0] / E_s, in scene order.  One workgroup, S <= kT.
template <int kStats>
__global__ __launch_bounds__(kT) void seg_total_kernel(const float* __restrict__ part, int S,
                                                       const int32_t* __restrict__ eoff,
                                                       const float* __restrict__ weight, float* __restrict__ tot,
                                                       float* __restrict__ loss) {
  __shared__ float sh[kT];
  const int s = threadIdx.x;
  if (s < S) {
    float a[kStats];
#pragma unroll
    for (int i = 0; i < kStats; ++i) a[i] = 0.f;
    for (int g = 0; g < kSegG; ++g)
#pragma unroll
      for (int i = 0; i < kStats; ++i) a[i] += part[kStats * (int64_t(s) * kSegG + g) + i];
#pragma unroll
    for (int i = 0; i < kStats; ++i) tot[kStats * s + i] = a[i];
    sh[s] = a[0];
  }
  __syncthreads();
  if (loss && threadIdx.x == 0) {
    float L = 0.f;
    for (int q = 0; q < S; ++q) {
      const float w = weight[q];
      if (w != 0.f) L += w * (sh[q] / float(eoff[q + 1] - eoff[q]));
    }
    loss[0] = L;
  }
}

// the scale of camera / point i's scene; skip = a scene of weight 0
struct SegScale {
  bool skip;
  EdgeScale k;
};

template <class Term, bool kSeg>
__device__ __forceinline__ SegScale seg_scale(int64_t E_norm, const int32_t* __restrict__ eoff,
                                              const int32_t* __restrict__ scene_of, int64_t i,
                                              const float* __restrict__ weight, const float* __restrict__ dloss,
                                              const float* __restrict__ tot) {
  if constexpr (!kSeg) {
    return {false, Term::scales(dloss[0], float(E_norm), tot, 0)};
  } else {
    const int s = scene_of[i];
    const float w = weight[s];
    return {w == 0.f, Term::scales(dloss[0] * w, float(eoff[s + 1] - eoff[s]), tot, s)};
  }
}

// dP_c over camera c = blockIdx.x's contiguous edge range [cptr[c], cptr[c+1]) by the workgroup.
// kSeg: the scale is the one of the camera's scene (eoff, scene_of_cam, weight); else of E_norm edges.
template <class Term, bool kSeg>
__global__ __launch_bounds__(kT) void edge_bwd_cam_kernel(
    const int32_t* __restrict__ cptr, const int32_t* __restrict__ pt, const float* __restrict__ vals, int64_t E_norm,
    const int32_t* __restrict__ eoff, const int32_t* __restrict__ scene_of_cam, const float* __restrict__ weight,
    const float* __restrict__ P, const float* __restrict__ X, int64_t n, Term term, const float* __restrict__ dloss,
    const float* __restrict__ tot, float* __restrict__ dP) {
  __shared__ float sh[kT / 64 * 12];
  const int c = blockIdx.x;
  const SegScale sc = seg_scale<Term, kSeg>(E_norm, eoff, scene_of_cam, c, weight, dloss, tot);
  if (sc.skip) {
    if (threadIdx.x < 12) dP[int64_t(c) * 12 + threadIdx.x] = 0.f;
    return;
  }
  float acc[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) acc[i] = 0.f;
  for (int e = cptr[c] + threadIdx.x; e < cptr[c + 1]; e += kT) {
    const float2 m = reinterpret_cast<const float2*>(vals)[e];
    float y[3], xs[4], g[3];
    project(P, X, n, c, pt[e], y, xs);
    term.grad(y, m.x, m.y, sc.k, g);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[4 * i + j] = fmaf(g[i], xs[j], acc[4 * i + j]);
  }
  const float s = block_sums(acc, sh);
  if (threadIdx.x < 12) dP[int64_t(c) * 12 + threadIdx.x] = s;
}

// d pts3D[:, p] over point p's edges in CSR order (perm: edge ids, null = the edges' own order);
// one thread per point
template <class Term, bool kSeg>
__global__ __launch_bounds__(kT) void edge_bwd_pt_kernel(
    const int32_t* __restrict__ pptr, const int32_t* __restrict__ perm, const int32_t* __restrict__ cam,
    const float* __restrict__ vals, int64_t E_norm, const int32_t* __restrict__ eoff,
    const int32_t* __restrict__ scene_of_pt, const float* __restrict__ weight, const float* __restrict__ P,
    const float* __restrict__ X, int64_t n, Term term, const float* __restrict__ dloss,
    const float* __restrict__ tot, float* __restrict__ dX) {
  const int64_t p = int64_t(blockIdx.x) * kT + threadIdx.x;
  if (p >= n) return;
  const SegScale sc = seg_scale<Term, kSeg>(E_norm, eoff, scene_of_pt, p, weight, dloss, tot);
  float a[4] = {0.f, 0.f, 0.f, 0.f};
  if (!sc.skip)
    for (int q = pptr[p]; q < pptr[p + 1]; ++q) {
      const int e = perm ? perm[q] : q;
      const float2 m = reinterpret_cast<const float2*>(vals)[e];
      const int c = cam[e];
      float y[3], xs[4], g[3];
      project(P, X, n, c, p, y, xs);
      term.grad(y, m.x, m.y, sc.k, g);
      const float* pc = P + int64_t(c) * 12;
#pragma unroll
      for (int j = 0; j < 4; ++j) a[j] = fmaf(pc[j], g[0], fmaf(pc[4 + j], g[1], fmaf(pc[8 + j], g[2], a[j])));
    }
#pragma unroll
  for (int j = 0; j < 4; ++j) dX[j * n + p] = a[j];
}

// ---- launchers: the argument checks of the extern "C" entries, once.  vals is read as float2.
inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

template <class Term, bool kEdgeOut = false>
int launch_fwd(const char* name, const int32_t* cam, const int32_t* pt, const float* vals, int64_t E, const float* P,
               const float* X, int64_t n, Term term, float* edge_out, float* part, void* stream) {
  GASFM_REQUIRE(E >= (Term::kIsLoss ? 1 : 0) && (E == 0 || n > 0), "%s: E=%lld n=%lld", name, (long long)E,
                (long long)n);
  GASFM_REQUIRE((E == 0 || (cam && pt && vals && P && X)) && part, "%s: null pointer", name);
  GASFM_REQUIRE(aligned8(vals), "%s: vals must be 8-byte aligned", name);
  hipLaunchKernelGGL((edge_fwd_kernel<Term, kEdgeOut>), dim3(part_rows(E)), dim3(kT), 0,
                     reinterpret_cast<hipStream_t>(stream), cam, pt, vals, E, P, X, n, term, edge_out, part);
  return launch_status(name);
}

// weight / loss: the batch total of a loss; both null for a metric
template <class Term>
int launch_seg_fwd(const char* name, const int32_t* cam, const int32_t* pt, const float* vals, const int32_t* eoff,
                   int32_t S, const float* weight, const float* P, const float* X, int64_t n, Term term, float* part,
                   float* tot, float* loss, void* stream) {
  GASFM_REQUIRE(S > 0 && S <= kT && n > 0, "%s: S=%d n=%lld", name, S, (long long)n);
  GASFM_REQUIRE(cam && pt && vals && eoff && P && X && part && tot && (!Term::kIsLoss || (weight && loss)),
                "%s: null pointer", name);
  GASFM_REQUIRE(aligned8(vals), "%s: vals must be 8-byte aligned", name);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(edge_fwd_seg_kernel<Term>, dim3(kSegG, S), dim3(kT), 0, st, cam, pt, vals, eoff, P, X, n, term,
                     part);
  hipLaunchKernelGGL(seg_total_kernel<Term::kStats>, dim3(1), dim3(kT), 0, st, part, S, eoff, weight, tot,
                     Term::kIsLoss ? loss : nullptr);
  return launch_status(name);
}

// The scenes of a union batch (kSeg); one scene of E edges, normalised by E_norm >= E, otherwise.
struct Scenes {
  const int32_t* eoff;
  int32_t S;
  const int32_t *of_cam, *of_pt;
  const float* weight;
};

template <class Term, bool kSeg>
int launch_bwd(const char* name, const int32_t* cam_ptr, int32_t m, const int32_t* pt_ptr, const int32_t* perm,
               const int32_t* cam, const int32_t* pt, const float* vals, int64_t E, int64_t E_norm, const Scenes& sc,
               const float* P, const float* X, int64_t n, Term term, const float* dloss, const float* tot, float* dP,
               float* dX, void* stream) {
  if constexpr (kSeg) {
    GASFM_REQUIRE(sc.S > 0 && m > 0 && n > 0, "%s: S=%d m=%d n=%lld", name, sc.S, m, (long long)n);
    GASFM_REQUIRE(sc.eoff && sc.of_cam && sc.of_pt && sc.weight, "%s: null pointer", name);
  } else {
    GASFM_REQUIRE(E > 0 && n > 0 && m > 0 && E_norm >= E, "%s: E=%lld E_norm=%lld m=%d n=%lld", name, (long long)E,
                  (long long)E_norm, m, (long long)n);
  }
  GASFM_REQUIRE(cam_ptr && pt_ptr && cam && pt && vals && P && X && dloss && dP && dX &&
                    (tot || !Term::kGradReadsTot),
                "%s: null pointer", name);
  GASFM_REQUIRE(aligned8(vals), "%s: vals must be 8-byte aligned", name);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL((edge_bwd_cam_kernel<Term, kSeg>), dim3(m), dim3(kT), 0, st, cam_ptr, pt, vals, E_norm, sc.eoff,
                     sc.of_cam, sc.weight, P, X, n, term, dloss, tot, dP);
  hipLaunchKernelGGL((edge_bwd_pt_kernel<Term, kSeg>), dim3(unsigned((n + kT - 1) / kT)), dim3(kT), 0, st, pt_ptr,
                     perm, cam, vals, E_norm, sc.eoff, sc.of_pt, sc.weight, P, X, n, term, dloss, tot, dX);
  return launch_status(name);
}

}  // namespace gasfm

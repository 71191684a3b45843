/*
 * gasfm_edge_wide.h — C ABI of the 32 -> 128 edge epilogue of a depth conf's last block
 * (gasfm_amd/csrc/edge_wide.hip, gfx950).
 *
 * Reference: code/models/layers.py:232-261 and 911-956 for the last GraphAttnSfMLayer of a conf
 * with a depth head (n_feat_proj 32 in, model.depth_head.n_feat = 128 out):
 *   P'[e] = Wsk relu(LN_b(P[e])) + bsk
 *         + scale*(Wp [relu(LN_a(P[e])) | P0[e]] + bp + Sp[pt[e]] + Sv[cam[e]] + Sg),  scale = 1/4.
 *
 * Same conventions as gasfm.h (status codes, caller-allocated device buffers; `items` points at
 * gasfm_work_item records, declared void* so that this header parses on its own,
 * `stream` a hipStream_t passed as void*, deterministic reductions); the entry points are part of
 * the same libgasfm.so.  This header is written in gasfm.h's grammar: gasfm_amd/edge_wide/_binding.py reads
 * the binding from it.
 */
#ifndef GASFM_EDGE_WIDE_H
#define GASFM_EDGE_WIDE_H

#include <stdint.h>

#include "gasfm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Launch geometry and partial-row shape.  which = 0: the forward's launch for E edges: returns its
 * workgroups (0 when E <= 0), *cols = the edges one workgroup takes per pass of its tile loop.
 * which = 1: gasfm_edge_wide_epilogue_bwd's partial buffer for n_items camera work items: returns
 * its rows (one per workgroup; 0 when n_items <= 0), *cols = the row width
 * [dWp 128 x ldWp | dWsk 128 x 32 | dbsk 128 | dgamma_a 32 | dbeta_a 32 | dgamma_b 32 | dbeta_b 32]
 * (ldWp = 34 with P0, 32 without).  gasfm_colsum of the buffer gives the gradients. */
int32_t gasfm_edge_wide_part_shape(int32_t which, int64_t E, int32_t n_items, int32_t ldWp, int32_t* cols);

/* P'[e] [128] = Wsk relu(LN_b(P[e])) + bsk
 *             + scale*(Wp [relu(LN_a(P[e])) | P0[e]] + bp + Sp[pt[e]] + Sv[cam[e]] + Sg).
 * Replaces (reference): the last GraphAttnSfMLayer of a conf with a depth head, layers.py:232-261
 * (both LayerNorm + ReLU, torch.cat with the init features, skip_projection and the residual add)
 * with GraphAttnSfMProjectionFeatureUpdate.forward, layers.py:911-956 (lin_proj, the two gathers of
 * 128-wide node rows, the global term and the / 4).  P [E x 32], P0 [E x 2] or NULL, Wp
 * [128 x ldWp] (ldWp = 34 with P0, 32 without), Wsk [128 x 32], Sp [n x 128], Sv rows ldSv >= 128
 * floats apart, Sg [128].  Both LayerNorms are required (NULL is refused). */
int gasfm_edge_wide_epilogue_fwd(const float* P, const float* P0, const int32_t* cam, const int32_t* pt,
                                 int64_t E, const float* ln_a_w, const float* ln_a_b, const float* ln_b_w,
                                 const float* ln_b_b, float eps, const float* Wp, int32_t ldWp,
                                 const float* bp, const float* Wsk, const float* bsk, const float* Sp,
                                 const float* Sv, int64_t ldSv, const float* Sg, float scale, float* Pout,
                                 void* stream);

/* Backward of the above over the camera work items (contiguous edges of one camera), from dPo
 * [E x 128]: dP [E x 32] = LN_a_bwd(mask_a scale Wp[:, :32]^T dPo) + LN_b_bwd(mask_b Wsk^T dPo)
 * (complete for this epilogue), dP0 [E x 2], dSv[cam] [128] (partials to part_dsv for split items)
 * and one partial row per workgroup (gasfm_edge_wide_part_shape, which = 1).
 * Replaces (reference): autograd's backward of the ops listed at gasfm_edge_wide_epilogue_fwd: two
 * LayerNorm backwards, the index_add scatter of view_features[cam] (layers.py:940) and the K = E
 * weight-gradient GEMMs of lin_proj and skip_projection. */
int gasfm_edge_wide_epilogue_bwd(const void* items, int32_t n_items, const float* dPo,
                                 const float* P, const float* P0, const float* ln_a_w, const float* ln_a_b,
                                 const float* ln_b_w, const float* ln_b_b, float eps, const float* Wp,
                                 int32_t ldWp, const float* Wsk, float scale, float* dP, float* dP0,
                                 float* dSv, float* part_dsv, float* part, void* stream);

/* out[seg] = scale * sum_{edges of the item} X[src]  (128-wide rows, row stride ldX >= 128; src via
 * perm); items / part as gasfm_segment_rowsum.
 * Replaces (reference): the index_add scatter of scenepoint_features[pt] (layers.py:940) at the
 * depth conf's last block. */
int gasfm_segment_rowsum_w(const void* items, int32_t n_items, const int32_t* perm,
                           const float* X, int64_t ldX, float scale, float* out, float* part,
                           void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GASFM_EDGE_WIDE_H */

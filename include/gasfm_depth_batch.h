/*
 * gasfm_depth_batch.h — C ABI of the depth branch over a union batch
 * (gasfm_amd/csrc/depth_batch.hip, gfx950): DirectDepthLoss, the depth scales and
 * the 2-view error of gasfm_depth_eval.h, per scene of a batch in one launch
 * sequence whose geometry depends on (E_cap, S) only.
 *
 * A union batch is the one of csrc/edge_loss.hpp: scene s owns the edges
 * [eoff[s], eoff[s+1]) of E_cap edges (eoff int32 [S + 1] on the device, read by
 * the kernels and clamped to [0, E_cap]); the batch value is
 * sum_s weight[s] * value_s and a padding scene has weight 0.  S <= 256.
 *
 * Every per-scene pass runs on a (GASFM_DEPTH_SEG_G, S) grid: workgroup (g, s)
 * walks edges eoff[s] + 256 g + t, + 256 GASFM_DEPTH_SEG_G, ... of scene s and
 * writes partial row s * GASFM_DEPTH_SEG_G + g; one workgroup then sums each
 * scene's rows in order.  No atomics, no host read: every entry can be captured
 * and two calls on equal inputs give equal bits.
 *
 * Same conventions as gasfm.h (status codes, caller-allocated device buffers,
 * `stream` a hipStream_t passed as void*); the entry points are part of the same
 * libgasfm.so.  This header is written in gasfm.h's grammar:
 * gasfm_amd/depth_batch/_binding.py reads the binding from it.
 */
#ifndef GASFM_DEPTH_BATCH_H
#define GASFM_DEPTH_BATCH_H

#include <stdint.h>

#include "gasfm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Workgroups (partial rows) per scene of every pass. */
#define GASFM_DEPTH_SEG_G 32

/* Rows of a partial buffer for S scenes ([rows, 2] floats; doubles for the scales). */
int32_t gasfm_depth_seg_part_rows(int32_t S);

/* DirectDepthLoss over a union batch (gasfm_depth_loss_* of gasfm.h per scene, the
 * per-edge arithmetic shared through csrc/depth_term.hpp).  a = predicted depths,
 * b = targets, both [E_cap].
 *   _seg_sums  sums [S, 2] = per scene (sum a, sum b)
 *   _seg_fwd   tot [S, 2] = per scene (sum l_e, sum g_e a_e);
 *              loss [1] = sum_s weight[s] * tot[s][0] / E_s in scene order
 *   _seg_bwd   da [E_cap] = d loss / d a * dloss[0], from E_s, sums[s], tot[s] and
 *              dloss[0] * weight[s] of the edge's scene (the same slice walk: no
 *              scene-of-edge table)
 * A scene of weight 0 writes zero partial rows / zero gradients and reads neither
 * a, b nor its sums: NaN there reaches no output.  Such a scene may be empty.  A
 * scene of nonzero weight and no edges makes the loss NaN (the reference's mean
 * of nothing).  Edges outside [eoff[0], eoff[S]) are not written by _seg_bwd.
 * part: gasfm_depth_seg_part_rows(S) x 2 floats of scratch. */
int gasfm_depth_loss_seg_sums(const float* a, const float* b, const int32_t* eoff, int32_t S,
                              int64_t E_cap, const float* weight, float* part, float* sums,
                              void* stream);
int gasfm_depth_loss_seg_fwd(const float* a, const float* b, const int32_t* eoff, int32_t S,
                             int64_t E_cap, const float* weight, const float* sums, int32_t l2,
                             float* part, float* tot, float* loss, void* stream);
int gasfm_depth_loss_seg_bwd(const float* a, const float* b, const int32_t* eoff, int32_t S,
                             int64_t E_cap, const float* weight, const float* sums, const float* tot,
                             int32_t l2, const float* dloss, float* da, void* stream);

/* scales [S, 2] floats = per scene (mean dp, mean dg): an fp64 fixed-order sum
 * divided by E_s and rounded to float32 (gasfm_depth_norm_stats per scene).  NaN
 * propagates; a scene without edges gives NaN.  ws: gasfm_depth_seg_part_rows(S) x 2
 * doubles. */
int gasfm_depth_scales_seg(const float* dp, const float* dg, const int32_t* eoff, int32_t S,
                           int64_t E_cap, double* ws, float* scales, void* stream);

/* gasfm_backproj_2view with the rescale factor scales[s][1] / scales[s][0] of the
 * destination edge's scene; tot [S, 2] = per scene (sum of the non-NaN errors,
 * their count).  cam, pt, src, d [E_cap], xy [E_cap, 2] (8-byte aligned), camtab
 * [m, GASFM_CAMTAB_FLOATS] (16-byte aligned) hold union indices.  src[e'] outside
 * [0, E_cap), a camera outside [0, m) or (pt given) pt[e] != pt[e'] is not
 * followed: NaN, left out of the count.  err and rdepth ([E_cap], written inside
 * [eoff[0], eoff[S]) only) may each be NULL. */
int gasfm_backproj_2view_seg(const int32_t* cam, const int32_t* pt, const float* xy, const float* d,
                             const float* scales, const int32_t* src, const int32_t* eoff, int32_t S,
                             int64_t E_cap, const float* camtab, int32_t m, float* err, float* rdepth,
                             float* part, float* tot, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GASFM_DEPTH_BATCH_H */

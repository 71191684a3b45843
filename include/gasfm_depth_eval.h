/*
 * gasfm_depth_eval.h — C ABI of the depth-head evaluation (gasfm_amd/csrc/depth_eval.hip, gfx950).
 *
 * Reference: code/evaluation.py:33-72, 241-301 with
 * geo_utils.reprojection_error_backproj_random_view_pairs (geo_utils.py:393-464),
 * general_utils.shuffle_coo_matrix_along_axis_while_preserving_sparsity_pattern and
 * geo_utils.determine_depth_scale (geo_utils.py:782-833).  The reference works on dense
 * [m, n, 3] fp64 arrays on the host; here every quantity is per visibility edge
 * e = (camera, point), in the edge order of the scene.
 *
 * Same conventions as gasfm.h (status codes, caller-allocated device buffers,
 * `stream` a hipStream_t passed as void*); the entry points are part of the same
 * libgasfm.so.  This header is written in gasfm.h's grammar:
 * gasfm_amd/depth_eval/_binding.py reads the binding from it.
 *
 * No entry point reads device memory on the host, array sizes depend on (E, m, n)
 * only, and no kernel uses an atomic: every call can be captured, and two calls on
 * equal inputs give equal bits.
 */
#ifndef GASFM_DEPTH_EVAL_H
#define GASFM_DEPTH_EVAL_H

#include <stdint.h>

#include "gasfm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Floats per camera of the table gasfm_backproj_2view reads: [R | t] [12] | K^-1 [9] |
 * K [9], each row-major, | 2 of padding (rows are 128 bytes, read as float4). */
#define GASFM_CAMTAB_FLOATS 32

/* Track pairing.  Point p's track is the edges perm[pt_ptr[p] .. pt_ptr[p+1])
 * (perm NULL: the positions themselves, as in gasfm_depth_stats).  The edges of a
 * track are ranked by (key, edge id); src[edge of rank r] = edge of rank r - 1,
 * and rank 0 takes the last: one cycle of the track's length L >= 2, uniformly
 * distributed for independent uniform keys.  A track of length 1 gets src = -1
 * and is counted in bad[0]; an empty track is skipped.  A CSR entry outside
 * [0, E) is neither read nor written.  Any L: a wave per track, 64 x 64 exchanges
 * of (key, id) between lanes.  Two launches (pairing, count). */
int gasfm_track_cycle(const int32_t* pt_ptr, const int32_t* perm, const int32_t* key, int64_t E,
                      int64_t n, int32_t* src, int32_t* bad, void* stream);

/* Rows of gasfm_backproj_2view's partial buffer ([rows, 2] floats). */
int32_t gasfm_backproj_2view_part_rows(int64_t E);

/* 2-view error.  For the destination edge e' = (c', p) with e = src[e'] = (c, p):
 *   x_n = K_c^-1 (u_e, v_e, 1) / its third coordinate
 *   X   = R_c^T (scale[0] d_e (x_n, 1) - t_c)          (= R_c^T (...) + C_c)
 *   q   = R_c' X + t_c',  rdepth[e'] = q_z,  err[e'] = || xy_e' - pi(K_c' q) ||
 * camtab [m, GASFM_CAMTAB_FLOATS] (16-byte aligned), xy [E, 2] pixels (8-byte
 * aligned), d [E], scale a device scalar.  err and rdepth may each be NULL.
 * part [rows, 2] = per-workgroup (sum of the non-NaN err, their count) for
 * gasfm_colsum, as gasfm_reproj_error.  src[e'] outside [0, E), a camera outside
 * [0, m) or (pt given) pt[e] != pt[e'] is not followed: err = rdepth = NaN.
 * E = 0 writes the one zero partial row. */
int gasfm_backproj_2view(const int32_t* cam, const int32_t* pt, const float* xy, const float* d,
                         const float* scale, const int32_t* src, int64_t E, const float* camtab,
                         int32_t m, float* err, float* rdepth, float* part, void* stream);

/* Depth scales and normalised-depth statistics.
 *   scales [2] floats = mean(dp), mean(dg): an fp64 fixed-order sum divided by E
 *   and rounded to float32 (determine_depth_scale);
 *   stats [7] doubles = sum, min, max of float(dp / scales[0]);  sum, min, max of
 *   float(dg / scales[1]);  sum of | float(dp / s_p) - float(dg / s_g) |
 *   (fp32 divisions and difference, fp64 sums in a fixed order).
 * NaN propagates through sum, min and max (ndarray.mean / min / max).  dg NULL:
 * scales[1] and stats[3..6] are NaN.  stats NULL: only the scales (two launches
 * instead of four).  ws: gasfm_depth_norm_stats_ws_doubles(E) doubles.  E = 0:
 * every output is NaN and no input is read. */
int64_t gasfm_depth_norm_stats_ws_doubles(int64_t E);
int gasfm_depth_norm_stats(const float* dp, const float* dg, int64_t E, double* ws, float* scales,
                           double* stats, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GASFM_DEPTH_EVAL_H */

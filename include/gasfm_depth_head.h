/*
 * gasfm_depth_head.h — C ABI of the fused depth head (gasfm_amd/csrc/depth_head.hip, gfx950).
 *
 * Reference: code/models/graph_attn_sfm.py:153-162, the per-edge depth head
 * get_linear_layers([128, 128, 128, 1], norm=False) applied to the last block's
 * projection features:
 *   y1 = P W1^T + b1,  y2 = relu(y1) W2^T + b2,  d = relu(y2) . w3 + b3.
 *
 * Same conventions as gasfm.h (status codes, caller-allocated device buffers,
 * `stream` a hipStream_t passed as void*, deterministic reductions); the entry
 * points are part of the same libgasfm.so.  This header is written in gasfm.h's
 * grammar: gasfm_amd/depth_head/_binding.py reads the binding from it.
 *
 * Shapes: P [E, 128] row-major fp32, rows 16-byte aligned; W1, W2 [128, 128],
 * b1, b2 [128], W3 [1, 128], b3 [1]; d, dd [E].  E = 0 returns GASFM_OK without a
 * launch; a null or misaligned pointer with E > 0 returns GASFM_ERR_INVALID.
 */
#ifndef GASFM_DEPTH_HEAD_H
#define GASFM_DEPTH_HEAD_H

#include <stdint.h>

#include "gasfm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Partial-row shape of the backward's weight gradients: which = 0 part_a
 * (dW1 [128 x 128] | db1 [128]), 1 part_b (dW2 [128 x 128] | db2 [128] |
 * dW3 [128] | db3 [1]).  Returns the row count (one row per workgroup; 0 when
 * E <= 0) and the row width in *cols.  gasfm_colsum of a partial buffer gives
 * the gradients. */
int32_t gasfm_depth_head_part_shape(int64_t E, int32_t which, int32_t* cols);

/* d [E] = depth_head(P).  Nothing else is written. */
int gasfm_depth_head_fwd(const float* P, int64_t E, const float* W1, const float* b1,
                         const float* W2, const float* b2, const float* W3, const float* b3,
                         float* d, void* stream);

/* Backward from P and the weights (y1, y2 are recomputed): dP [E, 128] and the
 * two partial buffers of gasfm_depth_head_part_shape.  Two launches. */
int gasfm_depth_head_bwd(const float* P, int64_t E, const float* W1, const float* b1,
                         const float* W2, const float* b2, const float* W3, const float* dd,
                         float* dP, float* part_a, float* part_b, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GASFM_DEPTH_HEAD_H */

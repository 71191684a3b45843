"""The 32 -> 128 edge epilogue of a depth conf's last block (csrc/edge_wide.hip, include/gasfm_edge_wide.h):
the kernels' wrappers.  The autograd Function is edge_block.WideEpilogueFn, the route
GraphAttnSfMLayer.forward_fused_wide."""
from ._binding import epilogue_bwd, epilogue_fwd, functions, lib, part_shape, segment_rowsum_w  # noqa: F401

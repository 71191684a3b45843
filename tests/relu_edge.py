"""Keeping fp64-compared LayerNorm + ReLU cases off the ReLU edge (shared by the view-block,
view-chain and point-edge tests; a plain module like gemm_checks.py, not a fixture)."""
import torch
import torch.nn.functional as F

RELU_MARGIN = 1e-4


def off_relu_edge(x, gamma, beta, eps=1e-5):
    """beta, moved per column by at most 1e-2, so that no pre-activation LN(x) gamma + beta lies
    within RELU_MARGIN of 0.  The gradient of relu jumps there, and an fp32 pre-activation (x up to
    ~10: ~1e-6 of rounding through the row statistics and the affine) may land on the other side
    of an fp64 one.  Seen at m = 129, D = 256 without prev: one pre-activation of 2.2e-8; flipping
    that single mask in the fp64 composition moves d agg by 0.29924 of |ref| = 239.2, the very
    figure the kernel missed the 1e-4 bar by.  No fp32 code can be held to the bar at such an input,
    so the inputs keep 100x the rounding away from the edge; a column's <= 1000 values always
    leave a gap that wide within +-1e-2."""
    pre = F.layer_norm(x, x.shape[1:], None, None, eps) * gamma + beta
    bad = (pre.abs() < RELU_MARGIN).any(0)
    if bad.any():
        shifts = torch.linspace(-1e-2, 1e-2, 201, dtype=torch.float64)
        gap = (pre[:, bad, None] + shifts).abs().amin(0)  # [columns, shifts]
        beta = beta.clone()
        beta[bad] += shifts[gap.argmax(1)]
        pre = F.layer_norm(x, x.shape[1:], None, None, eps) * gamma + beta
    assert pre.abs().min().item() >= RELU_MARGIN
    return beta

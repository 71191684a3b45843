"""The per-edge depth head as one fused autograd Function (csrc/depth_head.hip).

Reference code/models/graph_attn_sfm.py:153-162: depths = depth_head(P) with depth_head =
get_linear_layers([128, 128, 128, 1], norm=False), i.e. Linear(128,128) ReLU Linear(128,128) ReLU
Linear(128,1) on the raw last-block projection features P [E, 128] (no ReLU before the first layer).

aten keeps two [E, 128] activations for the backward and allocates their gradients; DepthHeadFn
saves P and the weights only, recomputes the activations tile by tile in the backward, and the only
[E, 128] tensors left are P and dP.  Sizes depend on E alone and nothing is read back to the host,
so the op can sit inside a captured step.
"""
import torch

from .. import _native
from . import _binding
from ._binding import WIDTH

__all__ = ["DepthHeadFn", "fusable", "apply", "WIDTH"]


class DepthHeadFn(torch.autograd.Function):
    """P [E, 128] -> d [E, 1]: one forward kernel, two backward kernels that each recompute the
    forward (dW2 | db2 | dW3 | db3, then dP | dW1 | db1)."""

    @staticmethod
    def forward(ctx, P, W1, b1, W2, b2, W3, b3):
        E = P.shape[0]
        d = torch.empty((E, 1), dtype=torch.float32, device=P.device)
        _binding.fwd(P, W1, b1, W2, b2, W3, b3, d)
        ctx.save_for_backward(P, W1, b1, W2, b2, W3)
        ctx.defer = _native.defer_token(W1, b1, W2, b2, W3, b3)
        return d

    @staticmethod
    def backward(ctx, dd):
        P, W1, b1, W2, b2, W3 = ctx.saved_tensors
        E, F = P.shape[0], WIDTH
        ra, ca = _binding.part_shape(E, 0)
        rb, cb = _binding.part_shape(E, 1)
        dP = torch.empty((E, F), dtype=torch.float32, device=P.device)
        if E == 0:
            ta = torch.zeros(ca, dtype=torch.float32, device=P.device)
            tb = torch.zeros(cb, dtype=torch.float32, device=P.device)
        else:
            part_a = torch.empty((ra, ca), dtype=torch.float32, device=P.device)
            part_b = torch.empty((rb, cb), dtype=torch.float32, device=P.device)
            _binding.bwd(P, W1, b1, W2, b2, W3, dd.contiguous(), dP, part_a, part_b)
            ta, tb = _native.param_colsum(part_a, ctx.defer), _native.param_colsum(part_b, ctx.defer)
        dW1, db1 = ta[:F * F].view(F, F), ta[F * F:]
        o = F * F
        dW2, db2, dW3, db3 = tb[:o].view(F, F), tb[o:o + F], tb[o + F:o + 2 * F].view(1, F), tb[o + 2 * F:]
        return dP, dW1, db1, dW2, db2, dW3, db3


def _is_lin(m, i, o):
    return (isinstance(m, torch.nn.Linear) and m.in_features == i and m.out_features == o and m.bias is not None
            and all(t.dtype == torch.float32 and t.is_contiguous() and t.is_cuda for t in (m.weight, m.bias)))


def fusable(seq, P):
    """CUDA fp32 contiguous rows of width 128 and exactly Linear(128,128) ReLU Linear(128,128) ReLU
    Linear(128,1) -- two hidden layers, no norms -- with contiguous fp32 parameters on the device."""
    if not (isinstance(P, torch.Tensor) and P.is_cuda and P.dtype == torch.float32 and P.dim() == 2
            and P.shape[1] == WIDTH and P.is_contiguous()):
        return False
    if not isinstance(seq, torch.nn.Sequential) or len(seq) != 5:
        return False
    mods = list(seq)
    return (_is_lin(mods[0], WIDTH, WIDTH) and type(mods[1]) is torch.nn.ReLU and _is_lin(mods[2], WIDTH, WIDTH)
            and type(mods[3]) is torch.nn.ReLU and _is_lin(mods[4], WIDTH, 1))


def apply(seq, P):
    """seq(P) [E, 1] on the fused kernels; ``fusable(seq, P)`` must hold."""
    if not fusable(seq, P):
        raise ValueError("depth_head.apply: not the fp32 CUDA 128-128-128-1 head (check fusable() first)")
    l1, l2, l3 = seq[0], seq[2], seq[4]
    return DepthHeadFn.apply(P, l1.weight, l1.bias, l2.weight, l2.bias, l3.weight, l3.bias)

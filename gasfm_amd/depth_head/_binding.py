"""ctypes binding of include/gasfm_depth_head.h: the fused depth head's entry points in libgasfm.so.

The header is written in gasfm.h's grammar and read by the same parser (``_abi.parse``); its
signatures are set on the ``CDLL`` that ``_native.lib()`` returns.  The wrappers validate shape,
dtype and contiguity and raise on any failure: there is no fallback.
"""
import ctypes

import torch

from .. import _abi, _native
from ..build import DEPTH_HEAD_HEADER

WIDTH = 128

with open(DEPTH_HEAD_HEADER) as _f:
    functions, constants, structs = _abi.parse(_f.read())

_bound = None


def lib():
    """libgasfm.so with the header's signatures set."""
    global _bound
    L = _native.lib()
    if _bound is not L:
        for name, (res, args) in functions.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _bound = L
    return L


def part_shape(E, which):
    """(rows, cols) of a partial buffer: which = 0 dW1 | db1, 1 dW2 | db2 | dW3 | db3."""
    cols = ctypes.c_int32(0)
    rows = lib().gasfm_depth_head_part_shape(E, int(which), ctypes.byref(cols))
    return rows, cols.value


def _weights(W1, b1, W2, b2, W3, b3=None):
    shapes = ((W1, (WIDTH, WIDTH)), (b1, (WIDTH,)), (W2, (WIDTH, WIDTH)), (b2, (WIDTH,)), (W3, (1, WIDTH))) + \
        (((b3, (1,)),) if b3 is not None else ())
    for t, shape in shapes:
        if tuple(t.shape) != shape or not t.is_contiguous() or t.dtype != torch.float32 or not t.is_cuda:
            raise ValueError(f"depth head: weight {tuple(t.shape)} is not a contiguous fp32 CUDA {shape}")


def _vec(t, E, name):
    _native._req(t, name)
    if t.numel() != E or t.dim() not in (1, 2) or t.shape[0] != E:
        raise ValueError(f"{name}: expected {E} contiguous values, got {tuple(t.shape)}")


def fwd(P, W1, b1, W2, b2, W3, b3, d):
    """d [E] or [E, 1] = depth_head(P [E, 128])."""
    _native._req(P, "P", WIDTH)
    _weights(W1, b1, W2, b2, W3, b3)
    E = P.shape[0]
    _vec(d, E, "d")
    p = _native._p
    st = lib().gasfm_depth_head_fwd(p(P), E, p(W1), p(b1), p(W2), p(b2), p(W3), p(b3), p(d), _native._stream(P))
    _native.check(st, "gasfm_depth_head_fwd")


def bwd(P, W1, b1, W2, b2, W3, dd, dP, part_a, part_b):
    _native._req(P, "P", WIDTH)
    _native._req(dP, "dP", WIDTH)
    _weights(W1, b1, W2, b2, W3)
    E = P.shape[0]
    if dP.shape[0] != E:
        raise ValueError("depth_head.bwd: dP must be [E, 128]")
    _vec(dd, E, "dd")
    for part, which in ((part_a, 0), (part_b, 1)):
        _native._req(part, "part")
        if tuple(part.shape) != part_shape(E, which):
            raise ValueError("depth_head.bwd: partial buffer of the wrong shape")
    p = _native._p
    st = lib().gasfm_depth_head_bwd(p(P), E, p(W1), p(b1), p(W2), p(b2), p(W3), p(dd), p(dP), p(part_a), p(part_b),
                                    _native._stream(P))
    _native.check(st, "gasfm_depth_head_bwd")

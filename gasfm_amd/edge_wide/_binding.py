"""ctypes binding of include/gasfm_edge_wide.h: the 32 -> 128 edge epilogue of a depth conf's last
block (csrc/edge_wide.hip) in libgasfm.so.

The header is written in gasfm.h's grammar and read by the same parser (``_abi.parse``); its
signatures are set on the ``CDLL`` that ``_native.lib()`` returns.  Thin wrappers: they check dtype,
contiguity and widths and raise on any failure; there is no fallback.
"""
import ctypes

import torch

from .. import _abi, _native
from ..build import EDGE_WIDE_HEADER

with open(EDGE_WIDE_HEADER) as _f:
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

def part_shape(which, E, n_items=0, ldWp=34):
    """(rows, cols): which = 0 the forward's (workgroups, edges per workgroup pass), 1 the backward's
    partial buffer (gasfm.h)."""
    cols = ctypes.c_int32(0)
    rows = lib().gasfm_edge_wide_part_shape(which, E, n_items, ldWp, ctypes.byref(cols))
    return int(rows), cols.value


def _rows128(t, name):
    if not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 128 or t.stride(1) != 1 \
            or (t.shape[0] > 1 and t.stride(0) < 128):
        raise TypeError(f"{name}: expected [rows, 128] float32 CUDA rows with unit column stride")
    return t.stride(0) if t.shape[0] > 1 else 128


def epilogue_fwd(P, P0, cam, pt, lna_w, lna_b, lnb_w, lnb_b, eps, Wp, bp, Wsk, bsk, Sp, Sv, Sg, scale, out):
    _native._req(P, "P", 32)
    for t, n, cols in ((Sp, "Sp", 128), (Sg, "Sg", None), (Wp, "Wp", None), (Wsk, "Wsk", 32), (out, "P'", 128)):
        _native._req(t, n, cols)
    ldSv = _rows128(Sv, "Sv")
    st = lib().gasfm_edge_wide_epilogue_fwd(_native._p(P), _native._p(P0), _native._p(cam), _native._p(pt), P.shape[0], _native._p(lna_w), _native._p(lna_b),
                                            _native._p(lnb_w), _native._p(lnb_b), eps, _native._p(Wp), Wp.shape[1], _native._p(bp), _native._p(Wsk), _native._p(bsk),
                                            _native._p(Sp), _native._p(Sv), ldSv, _native._p(Sg), scale, _native._p(out), _native._stream(P))
    _native.check(st, "gasfm_edge_wide_epilogue_fwd")


def epilogue_bwd(items, n_items, dPo, P, P0, lna_w, lna_b, lnb_w, lnb_b, eps, Wp, Wsk, scale, dP, dP0, dSv,
                           part_dsv, part):
    _native._req(dPo, "dP'", 128)
    _native._req(P, "P", 32)
    st = lib().gasfm_edge_wide_epilogue_bwd(_native._p(items), n_items, _native._p(dPo), _native._p(P), _native._p(P0), _native._p(lna_w), _native._p(lna_b),
                                            _native._p(lnb_w), _native._p(lnb_b), eps, _native._p(Wp), Wp.shape[1], _native._p(Wsk), scale, _native._p(dP),
                                            _native._p(dP0), _native._p(dSv), _native._p(part_dsv), _native._p(part), _native._stream(dPo))
    _native.check(st, "gasfm_edge_wide_epilogue_bwd")


def segment_rowsum_w(items, n_items, perm, X, scale, out, part):
    st = lib().gasfm_segment_rowsum_w(_native._p(items), n_items, _native._p(perm), _native._p(X), X.stride(0), scale, _native._p(out), _native._p(part),
                                      _native._stream(X))
    _native.check(st, "gasfm_segment_rowsum_w")

"""ctypes binding of include/gasfm_depth_eval.h: the depth-head evaluation's entry points in libgasfm.so.

The header is written in gasfm.h's grammar and read by the same parser (``_abi.parse``); its
signatures are set on the ``CDLL`` that ``_native.lib()`` returns.  The wrappers validate shape,
dtype and contiguity and raise on any failure: there is no fallback.
"""
import torch

from .. import _abi, _native
from ..build import DEPTH_EVAL_HEADER

with open(DEPTH_EVAL_HEADER) as _f:
    functions, constants, structs = _abi.parse(_f.read())

CAMTAB_FLOATS = constants["GASFM_CAMTAB_FLOATS"]

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


def _i32(t, name, size=None):
    _native._i32vec(t, name)
    if size is not None and t.shape[0] != size:
        raise ValueError(f"{name}: expected {size} entries, got {t.shape[0]}")


def _f32(t, name, shape):
    _native._req(t, name)
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected {tuple(shape)}, got {tuple(t.shape)}")


def track_cycle(pt_ptr, perm, key):
    """(src [E] int32, bad [1] int32) of gasfm_track_cycle; the edges no track holds keep -1."""
    E, n = key.shape[0], pt_ptr.shape[0] - 1
    _i32(pt_ptr, "pt_ptr"), _i32(key, "key")
    if perm is not None:
        _i32(perm, "perm", E)
    src = torch.full((E,), -1, dtype=torch.int32, device=key.device)
    bad = torch.empty(1, dtype=torch.int32, device=key.device)
    p = _native._p
    st = lib().gasfm_track_cycle(p(pt_ptr), p(perm), p(key), E, n, p(src), p(bad), _native._stream(key))
    _native.check(st, "gasfm_track_cycle")
    return src, bad


def backproj_2view(cam, pt, xy, d, scale, src, camtab, err=None, rdepth=None):
    """Per-workgroup (sum, count) of the non-NaN 2-view errors ([rows, 2], for ``_native.colsum``);
    ``err`` / ``rdepth`` ([E] float32) are filled when given.  ``pt`` None: src is trusted to stay
    within its track."""
    E, m = cam.shape[0], camtab.shape[0]
    _i32(cam, "cam"), _i32(src, "src", E)
    if pt is not None:
        _i32(pt, "pt", E)
    _f32(xy, "xy", (E, 2)), _f32(d, "d", (E,)), _f32(camtab, "camtab", (m, CAMTAB_FLOATS))
    _native._req(scale, "scale")
    if scale.numel() != 1:
        raise ValueError("backproj_2view: scale must hold one value")
    for t, name in ((err, "err"), (rdepth, "rdepth")):
        if t is not None:
            _f32(t, name, (E,))
    L = lib()
    part = torch.empty((L.gasfm_backproj_2view_part_rows(E), 2), dtype=torch.float32, device=cam.device)
    p = _native._p
    st = L.gasfm_backproj_2view(p(cam), p(pt), p(xy), p(d), p(scale), p(src), E, p(camtab), m, p(err), p(rdepth),
                                p(part), _native._stream(cam))
    _native.check(st, "gasfm_backproj_2view")
    return part


def depth_norm_stats(dp, dg, stats=True):
    """(scales [2] float32, stats [7] float64 or None) of gasfm_depth_norm_stats."""
    E = dp.shape[0]
    _f32(dp, "dp", (E,))
    if dg is not None:
        _f32(dg, "dg", (E,))
    L = lib()
    dev = dp.device
    ws = torch.empty(int(L.gasfm_depth_norm_stats_ws_doubles(E)), dtype=torch.float64, device=dev)
    scales = torch.empty(2, dtype=torch.float32, device=dev)
    out = torch.empty(7, dtype=torch.float64, device=dev) if stats else None
    p = _native._p
    st = L.gasfm_depth_norm_stats(p(dp), p(dg), E, p(ws), p(scales), p(out), _native._stream(dp))
    _native.check(st, "gasfm_depth_norm_stats")
    return scales, out

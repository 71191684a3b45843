"""ctypes binding of include/gasfm_depth_batch.h: the depth branch's union-batch entry points in libgasfm.so.

The header is written in gasfm.h's grammar and read by the same parser (``_abi.parse``); its
signatures are set on the ``CDLL`` that ``_native.lib()`` returns.  The wrappers validate shape,
dtype and contiguity and raise on any failure: there is no fallback.
"""
import torch

from .. import _abi, _native
from ..build import DEPTH_BATCH_HEADER
from ..depth_eval._binding import CAMTAB_FLOATS

with open(DEPTH_BATCH_HEADER) as _f:
    functions, constants, structs = _abi.parse(_f.read())

SEG_G = constants["GASFM_DEPTH_SEG_G"]

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


def _f32(t, name, shape):
    _native._req(t, name)
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected {tuple(shape)}, got {tuple(t.shape)}")


def _i32(t, name, size):
    _native._i32vec(t, name)
    if t.shape[0] != size:
        raise ValueError(f"{name}: expected {size} entries, got {t.shape[0]}")


def _batch(a, b, eoff, weight, names):
    """(E_cap, S) of two [E_cap] float32 vectors over the scenes eoff [S + 1] (weight [S] or None)."""
    E = a.shape[0]
    _f32(a, names[0], (E,)), _f32(b, names[1], (E,))
    S = eoff.shape[0] - 1
    if S < 1 or S > 256:
        raise ValueError(f"eoff: expected 2 to 257 offsets, got {eoff.shape[0]}")
    _i32(eoff, "eoff", S + 1)
    if weight is not None:
        _f32(weight, "weight", (S,))
    return E, S


def _part(L, S, dev, dtype=torch.float32):
    return torch.empty((L.gasfm_depth_seg_part_rows(S), 2), dtype=dtype, device=dev)


def depth_loss_seg_fwd(a, b, eoff, weight, l2):
    """(loss [1], sums [S, 2], tot [S, 2]) of gasfm_depth_loss_seg_sums + gasfm_depth_loss_seg_fwd."""
    E, S = _batch(a, b, eoff, weight, ("depths", "depth targets"))
    L, dev, p = lib(), a.device, _native._p
    part = _part(L, S, dev)
    sums, tot = (torch.empty((S, 2), dtype=torch.float32, device=dev) for _ in range(2))
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    st = L.gasfm_depth_loss_seg_sums(p(a), p(b), p(eoff), S, E, p(weight), p(part), p(sums), _native._stream(a))
    _native.check(st, "gasfm_depth_loss_seg_sums")
    st = L.gasfm_depth_loss_seg_fwd(p(a), p(b), p(eoff), S, E, p(weight), p(sums), int(l2), p(part), p(tot), p(loss),
                                    _native._stream(a))
    _native.check(st, "gasfm_depth_loss_seg_fwd")
    return loss, sums, tot


def depth_loss_seg_bwd(a, b, eoff, weight, sums, tot, l2, dloss):
    """da [E_cap] of gasfm_depth_loss_seg_bwd; edges outside the scenes keep 0."""
    E, S = _batch(a, b, eoff, weight, ("depths", "depth targets"))
    _f32(sums, "sums", (S, 2)), _f32(tot, "tot", (S, 2)), _f32(dloss, "dloss", (1,))
    da = torch.zeros_like(a)
    p = _native._p
    st = lib().gasfm_depth_loss_seg_bwd(p(a), p(b), p(eoff), S, E, p(weight), p(sums), p(tot), int(l2), p(dloss), p(da),
                                        _native._stream(a))
    _native.check(st, "gasfm_depth_loss_seg_bwd")
    return da


def depth_scales_seg(dp, dg, eoff):
    """scales [S, 2] float32 of gasfm_depth_scales_seg."""
    E, S = _batch(dp, dg, eoff, None, ("dp", "dg"))
    L, dev, p = lib(), dp.device, _native._p
    ws = _part(L, S, dev, torch.float64)
    scales = torch.empty((S, 2), dtype=torch.float32, device=dev)
    st = L.gasfm_depth_scales_seg(p(dp), p(dg), p(eoff), S, E, p(ws), p(scales), _native._stream(dp))
    _native.check(st, "gasfm_depth_scales_seg")
    return scales


def backproj_2view_seg(cam, pt, xy, d, scales, src, eoff, camtab, err=None, rdepth=None):
    """tot [S, 2] = per scene (sum of the non-NaN 2-view errors, count); ``err`` / ``rdepth`` ([E_cap]
    float32) are filled inside the scenes when given.  ``pt`` None: src is trusted to stay within its track."""
    E, m, S = cam.shape[0], camtab.shape[0], eoff.shape[0] - 1
    if S < 1 or S > 256:
        raise ValueError(f"eoff: expected 2 to 257 offsets, got {eoff.shape[0]}")
    _i32(cam, "cam", E), _i32(src, "src", E), _i32(eoff, "eoff", S + 1)
    if pt is not None:
        _i32(pt, "pt", E)
    _f32(xy, "xy", (E, 2)), _f32(d, "d", (E,)), _f32(camtab, "camtab", (m, CAMTAB_FLOATS)), _f32(scales, "scales", (S, 2))
    for t, name in ((err, "err"), (rdepth, "rdepth")):
        if t is not None:
            _f32(t, name, (E,))
    L, dev, p = lib(), cam.device, _native._p
    part = _part(L, S, dev)
    tot = torch.empty((S, 2), dtype=torch.float32, device=dev)
    st = L.gasfm_backproj_2view_seg(p(cam), p(pt), p(xy), p(d), p(scales), p(src), p(eoff), S, E, p(camtab), m, p(err),
                                    p(rdepth), p(part), p(tot), _native._stream(cam))
    _native.check(st, "gasfm_backproj_2view_seg")
    return tot

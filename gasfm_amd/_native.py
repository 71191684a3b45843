"""ctypes binding of the gasfm C ABI (include/gasfm.h).

The HIP library is REQUIRED: if ``libgasfm.so`` is missing or fails to load,
importing the compute entry points raises — there is no CPU or PyTorch
fallback for the attention path.  Host-only entry points (graph
preprocessing) work without a GPU, so DataLoader workers can use them.

Nothing here restates the header: every signature, struct layout and constant
comes from ``_abi``, which parses include/gasfm.h at import.  A new entry point
is declared in gasfm.h, defined in csrc/ and wrapped here; there is no table to
extend.
"""
import ctypes
import threading
import os

import numpy as np
import torch

from . import _abi
from .build import LIB

_C = _abi.constants
GASFM_OK, GASFM_ERR_INVALID, GASFM_ERR_OOM, GASFM_ERR_HIP, GASFM_ERR_UNSUPPORTED = (
    _C[k] for k in ("GASFM_OK", "GASFM_ERR_INVALID", "GASFM_ERR_OOM", "GASFM_ERR_HIP", "GASFM_ERR_UNSUPPORTED"))

_vp = ctypes.c_void_p
_i32 = ctypes.c_int32
_i64 = ctypes.c_int64

_SIGS = _abi.functions  # name -> (restype, argtypes)

_lib = None


def lib():
    """Load libgasfm.so (raising loudly if absent)."""
    global _lib
    if _lib is None:
        path = os.environ.get("GASFM_LIB") or LIB  # GASFM_LIB: an A/B build variant (build.build(out=...))
        if not os.path.exists(path):
            raise ImportError(
                f"gasfm native library not built: {path} missing. Run `python -m gasfm_amd.build` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        L = ctypes.CDLL(path)
        for name, (res, args) in _SIGS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def exported_symbols():
    return list(_SIGS)


def check(status, what):
    if status == GASFM_OK:
        return
    msg = lib().gasfm_last_error().decode(errors="replace")
    if status == GASFM_ERR_OOM:
        raise torch.OutOfMemoryError(f"{what}: {msg}")
    raise RuntimeError(f"{what} failed (status {status}): {msg}")


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(t):
    if _RAW_STREAM is not None and t.device.index is not None:
        # the current stream's handle without building a torch.cuda.Stream object (~2 us per
        # launch on the host: ~4,700 launches per eager training step)
        return ctypes.c_void_p(_RAW_STREAM(t.device.index))
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


# ---------------------------------------------------------------- kernel-choice record, tuning
def _enum(prefix):
    """{lower-cased member name without the prefix: value} of an enum of gasfm.h, its _COUNT aside."""
    return {k[len(prefix):].lower(): v for k, v in _C.items() if k.startswith(prefix) and k != prefix + "COUNT"}


KERNELS = _enum("GASFM_K_")  # "attn_fwd_grp": 0, ... "sos_edge_dw": 19
TUNING = _enum("GASFM_TUNE_")  # "attn_grp_rows": 0, ... "attn_grp_split": 4


def dispatch_counts():
    """{kernel name: launches since the last reset} of the size-dependent dispatches."""
    n = _C["GASFM_K_COUNT"]
    buf = (_i64 * n)()
    lib().gasfm_dispatch_counts(buf, n)
    return {k: int(buf[i]) for k, i in KERNELS.items()}


def dispatch_reset():
    lib().gasfm_dispatch_reset()


def tuning_get(key):
    return float(lib().gasfm_tuning_get(TUNING[key]))


def tuning_set(key, value):
    check(lib().gasfm_tuning_set(TUNING[key], float(value)), "gasfm_tuning_set")


class tuned:
    """Context manager: set dispatch thresholds, restore them on exit."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.prev = {k: tuning_get(k) for k in self.kv}
        for k, v in self.kv.items():
            tuning_set(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.prev.items():
            tuning_set(k, v)
        return False


class dispatch_record:
    """Context manager: ``rec.counts`` = launches per kernel inside the block."""

    def __enter__(self):
        self.start = dispatch_counts()
        return self

    def __exit__(self, *exc):
        end = dispatch_counts()
        self.counts = {k: end[k] - self.start[k] for k in end}
        return False


# ---------------------------------------------------------------- host graph preprocessing
def build_csr(key, n):
    """Stable counting sort of int32 keys in [0, n): returns (ptr[n+1], perm[E]) numpy int32."""
    key = np.ascontiguousarray(key, dtype=np.int32)
    E = key.shape[0]
    ptr = np.empty(n + 1, dtype=np.int32)
    perm = np.empty(max(E, 1), dtype=np.int32)
    st = lib().gasfm_build_csr(key.ctypes.data_as(_vp), E, n, ptr.ctypes.data_as(_vp),
                               perm.ctypes.data_as(_vp))
    check(st, "gasfm_build_csr")
    return ptr, perm[:E]


def plan_work(seg_ptr, max_piece, all_partial=False):
    """Split segments into work items; returns (items[n,4], combine[k,4], n_slots) numpy int32."""
    seg_ptr = np.ascontiguousarray(seg_ptr, dtype=np.int32)
    N = seg_ptr.shape[0] - 1
    ni, nc, ns = _i32(0), _i32(0), _i32(0)
    L = lib()
    L.gasfm_plan_work(seg_ptr.ctypes.data_as(_vp), N, max_piece, int(all_partial), None,
                      ctypes.byref(ni), None, ctypes.byref(nc), ctypes.byref(ns))
    items = np.empty((max(ni.value, 1), 4), dtype=np.int32)
    comb = np.empty((max(nc.value, 1), 4), dtype=np.int32)
    ni2, nc2 = _i32(ni.value), _i32(nc.value)
    st = L.gasfm_plan_work(seg_ptr.ctypes.data_as(_vp), N, max_piece, int(all_partial),
                           items.ctypes.data_as(_vp), ctypes.byref(ni2), comb.ctypes.data_as(_vp),
                           ctypes.byref(nc2), ctypes.byref(ns))
    check(st, "gasfm_plan_work")
    return items[:ni2.value], comb[:nc2.value], ns.value


# ---------------------------------------------------------------- device kernels
def attn_fwd(XL, XR, att, bias, perm, items, n_items, H, C, slope, finalize, out, seg_max, seg_sum, part=None,
             ldStat=None, lanes=False):
    """part: packed partial rows [slots, H*C + 2H] (acc | max | sum) or None.  lanes: the
    lane-per-item kernel (H = 4, C = 1; short items: block 0's point direction)."""
    ldStat = H if ldStat is None else ldStat
    fn = lib().gasfm_gat_attn_fwd_lanes if lanes else lib().gasfm_gat_attn_fwd
    st = fn(
        _p(XL), XL.stride(0), _p(XR), XR.stride(0), _p(att), _p(bias), _p(perm), _p(items), n_items, H, C,
        slope, int(finalize), _p(out), out.stride(0) if out is not None else 0, _p(seg_max), _p(seg_sum), ldStat,
        _p(part), _stream(XL))
    check(st, "gasfm_gat_attn_fwd")


def attn_combine(combine, n_combine, H, C, part, bias, finalize, out, seg_max, seg_sum, ldOut=None, ldStat=None):
    """Merge packed partial rows; out/seg_max/seg_sum may be views into a packed buffer (raw mode)."""
    ldOut = out.stride(0) if ldOut is None else ldOut
    ldStat = H if ldStat is None else ldStat
    st = lib().gasfm_gat_attn_combine(_p(combine), n_combine, H, C, _p(part), _p(bias), int(finalize), _p(out),
                                      ldOut, _p(seg_max), _p(seg_sum), ldStat, _stream(part))
    check(st, "gasfm_gat_attn_combine")


def attn_bwd_waves(n_items, H, C):
    return lib().gasfm_gat_attn_bwd_waves(n_items, H, C)


def attn_bwd(XL, XR, att, bias, perm, items, n_items, H, C, slope, out, seg_max, seg_sum, gout, dXL, dXR,
             part_dxr, datt_part, xl_by_position=False, lanes=False):
    fn = lib().gasfm_gat_attn_bwd_lanes if lanes else lib().gasfm_gat_attn_bwd
    st = fn(
        _p(XL), XL.stride(0), _p(XR), XR.stride(0), _p(att), _p(bias), _p(perm), _p(items), n_items, H, C,
        slope, _p(out), out.stride(0), _p(seg_max), _p(seg_sum), _p(gout), gout.stride(0), _p(dXL),
        dXL.stride(0), _p(dXR), dXR.stride(0), _p(part_dxr), _p(datt_part), int(xl_by_position), _stream(dXL))
    check(st, "gasfm_gat_attn_bwd")


def attn_bwd_combine(combine, n_combine, HC, part_dxr, dXR):
    st = lib().gasfm_gat_attn_bwd_combine(_p(combine), n_combine, HC, _p(part_dxr), _p(dXR), dXR.stride(0),
                                          _stream(dXR))
    check(st, "gasfm_gat_attn_bwd_combine")


def attn_bwd_combine2(combine, n_combine, HC, part_a, out_a, part_b, out_b):
    """attn_bwd_combine of two partial-row arrays over the same entries, one launch."""
    st = lib().gasfm_gat_attn_bwd_combine2(_p(combine), n_combine, HC, _p(part_a), _p(out_a), out_a.stride(0),
                                           _p(part_b), _p(out_b), out_b.stride(0), _stream(out_a))
    check(st, "gasfm_gat_attn_bwd_combine2")


_COUNTERS = {}
_COUNTER_POOL = 1 << 16


def _counters(device, n):
    """A range of n zeroed uint32 ticket counters for one colsum launch (self-resetting: the last
    arriver of each column chunk puts its counter back to 0).

    Every call gets its OWN range from a per-device pool, handed out round-robin, so colsums that
    run concurrently (on different streams, or on parallel branches of a captured graph) never
    share a ticket: a range comes back only after the other ~65k counters have been handed out.
    The pool is allocated once, large (a replacement allocated while a hipGraph is being captured
    would leave the nodes captured before it pointing at the freed array)."""
    n = max(1, int(n))
    if n > _COUNTER_POOL:
        raise ValueError(f"colsum counters: {n} requested, pool holds {_COUNTER_POOL}")
    c = _COUNTERS.get(device)
    if c is None:
        c = [torch.zeros(_COUNTER_POOL, dtype=torch.int32, device=device), 0]
        _COUNTERS[device] = c
    pool, at = c
    if at + n > _COUNTER_POOL:
        at = 0
    c[1] = at + n
    return pool[at:at + n]


def colsum(A, out=None):
    """Deterministic column sum of a 2-D fp32 CUDA tensor (row stride may exceed cols); one launch."""
    assert A.dim() == 2 and A.stride(1) == 1 and A.dtype == torch.float32
    rows, cols = A.shape
    if out is None:
        out = torch.empty(cols, dtype=torch.float32, device=A.device)
    L = lib()
    ws = torch.empty(int(L.gasfm_colsum_ws_floats(rows, cols)), dtype=torch.float32, device=A.device)
    cnt = _counters(A.device, L.gasfm_colsum_counters(cols))
    st = L.gasfm_colsum(_p(A), rows, cols, max(A.stride(0), cols), _p(ws), _p(out), _p(cnt), _stream(out))
    check(st, "gasfm_colsum")
    return out


def colsum_tall_ok(A):
    return (A.dim() == 2 and A.is_contiguous() and A.dtype == torch.float32
            and bool(lib().gasfm_colsum_tall_ok(A.shape[1])))


def colsum_tall(A, out=None):
    """Column sums of a contiguous tall [rows, cols] fp32 CUDA tensor (colsum_tall_ok)."""
    rows, cols = A.shape
    if out is None:
        out = torch.empty(cols, dtype=torch.float32, device=A.device)
    L = lib()
    ws = torch.empty(max(1, int(L.gasfm_colsum_tall_ws_floats(rows, cols))), dtype=torch.float32, device=A.device)
    cnt = _counters(A.device, 1)
    st = L.gasfm_colsum_tall(_p(A), rows, cols, _p(ws), _p(out), _p(cnt), _stream(out))
    check(st, "gasfm_colsum_tall")
    return out


def colsum_ranges(A, row_ptr, w=None, out=None):
    """[n_ranges, cols] fp64: out[s] = sum of w[r] * A[r] over rows row_ptr[s] <= r < row_ptr[s + 1]
    of a 2-D fp32 CUDA tensor (row stride may exceed cols).  row_ptr: int32 device row pointers
    within A's rows (not read here: no host synchronisation); w: fp64 [rows] or None.  One launch,
    ordered fp64 sums (csrc/colsum_ranges.hip)."""
    if not (A.is_cuda and A.dim() == 2 and A.dtype == torch.float32 and (A.shape[1] == 1 or A.stride(1) == 1)):
        raise ValueError("colsum_ranges: A must be a 2-D fp32 CUDA tensor with unit column stride")
    rows, cols = A.shape
    if cols < 1:
        raise ValueError("colsum_ranges: A has no columns")
    if row_ptr.dtype != torch.int32 or row_ptr.dim() != 1 or row_ptr.numel() < 1 or not row_ptr.is_contiguous() \
            or row_ptr.device != A.device:
        raise ValueError("colsum_ranges: row_ptr must be a contiguous int32 vector on A's device")
    n_ranges = row_ptr.numel() - 1
    if w is not None and not (w.dtype == torch.float64 and w.dim() == 1 and w.numel() == rows and w.is_contiguous()
                              and w.device == A.device):
        raise ValueError("colsum_ranges: w must be a contiguous fp64 vector with one entry per row of A")
    if out is None:
        out = torch.empty((n_ranges, cols), dtype=torch.float64, device=A.device)
    elif not (out.dtype == torch.float64 and tuple(out.shape) == (n_ranges, cols) and out.is_contiguous()
              and out.device == A.device):
        raise ValueError(f"colsum_ranges: out must be a contiguous fp64 [{n_ranges}, {cols}] tensor")
    ld = max(A.stride(0), cols) if rows > 1 else cols
    st = lib().gasfm_colsum_ranges(_p(A), ld, cols, _p(row_ptr), n_ranges, _p(w), _p(out), _stream(out))
    check(st, "gasfm_colsum_ranges")
    return out



# ---------------------------------------------------------------- batched weight-gradient sums
# A backward pass ends with ~150 column sums of per-workgroup weight-gradient partials (one per
# fused kernel).  Their results are parameter gradients that nothing reads before the backward
# pass returns, so inside a pass they are queued and run as ONE batched launch
# (gasfm_colsum_multi) from an autograd final callback: ~150 fewer kernel launches per step.
# Only when the model forward saw every parameter's .grad unset (AccumulateGrad then adopts the
# returned tensor instead of adding it to an existing gradient, so filling it later is safe);
# otherwise, and outside a backward pass, param_colsum is colsum.
_DEFER_FWD = False
_PENDING = {}
_SEEN = {}  # graph task -> ids of the parameters that already received a deferred sum in it
_PENDING_LOCK = threading.Lock()


def defer_token(*targets):
    """Captured by the fused Functions' forward (ctx.defer) and passed to param_colsum: in a
    deferring model forward, the tensors that receive the deferred sums when every one is a leaf
    (a parameter: no autograd node reads its gradient before the pass ends); else False."""
    if _DEFER_FWD and all(t is None or t.is_leaf for t in targets):
        return tuple(t for t in targets if t is not None) or True
    return False


class deferring_param_grads:
    """Set by GraphAttnSfMNet.forward for the duration of the forward."""

    def __init__(self, enabled):
        self.enabled = bool(enabled)

    def __enter__(self):
        global _DEFER_FWD
        self.prev, _DEFER_FWD = _DEFER_FWD, self.enabled
        return self

    def __exit__(self, *exc):
        global _DEFER_FWD
        _DEFER_FWD = self.prev
        return False


def param_colsum(A, defer):
    """colsum of weight-gradient partials; deferred to the end of the backward pass when
    ``defer`` (see above) and called inside one."""
    task = torch._C._current_graph_task_id() if defer else -1
    if task < 0:
        return colsum(A)
    if isinstance(defer, tuple) and any(t.grad is not None for t in defer):
        # the parameter already holds a gradient (retain_graph and a second backward, or two
        # forwards backpropagated separately): AccumulateGrad ADDS the returned tensor to it at
        # once, so it must be filled now
        return colsum(A)
    if isinstance(defer, tuple):
        # parameter -> the token (one per Function forward) whose sum it got first in this pass; the
        # same token again is another output of the same Function (e.g. both attention directions)
        with _PENDING_LOCK:
            seen = _SEEN.setdefault(task, {})
            again = any(seen.get(id(t), id(defer)) != id(defer) for t in defer)
            for t in defer:
                seen.setdefault(id(t), id(defer))
        if again and os.environ.get("GASFM_DEBUG_DEFER"):
            print("param_colsum: repeated targets", [tuple(t.shape) for t in defer], flush=True)
        if again:
            # a second contribution to these parameters in this pass (several forwards, one
            # backward: train.py sums the scenes' losses).  AccumulateGrad adopts one sum and adds
            # the other to it, so none may be left unfilled: fill the queued sums first (stream
            # order puts them before any later add), then sum this one now.
            _flush_param_colsums(task, final=False)
            return colsum(A)
    assert A.dim() == 2 and A.stride(1) == 1 and A.dtype == torch.float32
    rows, cols = A.shape
    L = lib()
    out = torch.empty(cols, dtype=torch.float32, device=A.device)
    ws = torch.empty(int(L.gasfm_colsum_ws_floats(rows, cols)), dtype=torch.float32, device=A.device)
    job = (A, ws, out, rows, cols, max(A.stride(0), cols), torch.cuda.current_stream(A.device))
    with _PENDING_LOCK:
        jobs = _PENDING.get(task)
        first = jobs is None
        if first:
            jobs = _PENDING[task] = []
        jobs.append(job)
    if first:
        torch.autograd.Variable._execution_engine.queue_callback(lambda: _flush_param_colsums(task))
    return out


def _flush_param_colsums(task, final=True):
    with _PENDING_LOCK:
        jobs = _PENDING.pop(task, [])
        if final:
            _SEEN.pop(task, None)
    if not jobs:
        return
    stream = jobs[0][6]
    assert all(j[6] == stream for j in jobs), "param_colsum: jobs queued on several streams"
    n = len(jobs)
    L = lib()
    arr = lambda ty, xs: (ty * n)(*xs)  # noqa: E731
    A = arr(ctypes.c_void_p, [j[0].data_ptr() for j in jobs])
    ws = arr(ctypes.c_void_p, [j[1].data_ptr() for j in jobs])
    out = arr(ctypes.c_void_p, [j[2].data_ptr() for j in jobs])
    rows = arr(ctypes.c_int64, [j[3] for j in jobs])
    cols = arr(ctypes.c_int32, [j[4] for j in jobs])
    ld = arr(ctypes.c_int64, [j[5] for j in jobs])
    dev = jobs[0][0].device
    cnt = _counters(dev, L.gasfm_colsum_multi_counters(n, cols))
    st = L.gasfm_colsum_multi(n, A, rows, cols, ld, ws, out, _p(cnt), ctypes.c_void_p(stream.cuda_stream))
    check(st, "gasfm_colsum_multi")
    # the partial buffers (jobs) are released only now, after the launch that reads them


# ---------------------------------------------------------------- fused per-edge block kernels
def _req(t, name, cols=None):
    if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
        raise TypeError(f"{name}: expected a contiguous float32 CUDA tensor (no CPU fallback)")
    if cols is not None and t.shape[-1] != cols:
        raise ValueError(f"{name}: expected {cols} columns, got {tuple(t.shape)}")


def edge_part_floats(which, E, n_items=0):
    return lib().gasfm_edge_part_floats(which, E, n_items)


def edge_prologue_fwd(P, ln_w, ln_b, eps, W, b, Y, pos=None, W2=None, b2=None):
    """W [64,32] / b [64], or the halves W [32,32] + W2 [32,32] and b [32] + b2 [32]."""
    _req(P, "P", 32)
    st = lib().gasfm_edge_prologue_fwd(_p(P), P.shape[0], _p(ln_w), _p(ln_b), eps, _p(W), _p(W2), _p(b), _p(b2),
                                       _p(Y), Y.stride(0), _p(pos), _stream(P))
    check(st, "gasfm_edge_prologue_fwd")


def _rows32(t, name):
    """[rows, 32] float32 CUDA rows with unit column stride (row stride >= 32: a column slice of a
    gathered [SV | XR] block is fine); returns the row stride."""
    if not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 32 or t.stride(1) != 1 \
            or (t.shape[0] > 1 and t.stride(0) < 32):
        raise TypeError(f"{name}: expected [rows, 32] float32 CUDA rows with unit column stride")
    return t.stride(0) if t.shape[0] > 1 else 32


def edge_epilogue_fwd(P, P0, cam, pt, ln_w, ln_b, eps, Wp, bp, Sp, Sv, Sg, scale, out):
    _req(P, "P", 32)
    for t, n in ((Sp, "Sp"), (Sg, "Sg"), (Wp, "Wp")):
        _req(t, n)
    ldSv = _rows32(Sv, "Sv")
    st = lib().gasfm_edge_epilogue_fwd(_p(P), _p(P0), _p(cam), _p(pt), P.shape[0], _p(ln_w), _p(ln_b), eps, _p(Wp),
                                       Wp.shape[1], _p(bp), _p(Sp), _p(Sv), ldSv, _p(Sg), scale, _p(out),
                                       _stream(P))
    check(st, "gasfm_edge_epilogue_fwd")


def edge_epilogue_bwd(items, n_items, dPo, P, P0, ln_w, ln_b, eps, Wp, scale, dSv, part_dsv, dP0, part_w):
    _req(dPo, "dP'", 32)
    st = lib().gasfm_edge_epilogue_bwd(_p(items), n_items, _p(dPo), _p(P), _p(P0), _p(ln_w), _p(ln_b), eps, _p(Wp),
                                       Wp.shape[1], scale, _p(dSv), _p(part_dsv), _p(dP0), _p(part_w), _stream(dPo))
    check(st, "gasfm_edge_epilogue_bwd")


def edge_prologue_bwd(dXL, P, dRes, ln_w, ln_b, eps, W, Wp, scale, dP, part, W2=None, dXLc=None):
    """dXLc: the camera half of dXL in its own [E, 32] buffer (dXL then holds the point half)."""
    _req(P, "P", 32)
    st = lib().gasfm_edge_prologue_bwd(_p(dXL), dXL.stride(0), _p(P), _p(dRes), P.shape[0], _p(ln_w), _p(ln_b), eps,
                                       _p(W), _p(W2), _p(Wp), Wp.shape[1] if Wp is not None else 0, scale, _p(dP),
                                       _p(part), _p(dXLc), dXLc.stride(0) if dXLc is not None else 0, _stream(P))
    check(st, "gasfm_edge_prologue_bwd")


def edge_cam_fwd(P, ln_w, ln_b, eps, Wpt, bpt, Wc, bc, XLp, pos, XR, att, bias, slope, plan_items, n_items,
                 finalize, out, seg_max, seg_sum, part, ldStat=4):
    """Edge prologue + camera-direction attention forward (csrc/edge_cam.hip): XLp [E, 32] (point
    half of lin_l, written through pos), camera aggregates into out / seg_max / seg_sum (complete
    items) or packed partial rows part [slots, 40]."""
    _req(P, "P", 32)
    ldXR = _rows32(XR, "XR")
    st = lib().gasfm_edge_cam_fwd(_p(P), _p(ln_w), _p(ln_b), eps, _p(Wpt), _p(bpt), _p(Wc), _p(bc), _p(XLp),
                                  XLp.stride(0), _p(pos), _p(XR), ldXR, _p(att), _p(bias), slope, _p(plan_items),
                                  n_items, int(finalize), _p(out), out.stride(0) if out is not None else 0,
                                  _p(seg_max), _p(seg_sum), ldStat, _p(part), _stream(P))
    check(st, "gasfm_edge_cam_fwd")


def _ld_stat(seg_max):
    """row stride of the [N, heads] statistics (4 for their own tensors; the partial-row stride when
    they are columns of a packed partial buffer)"""
    return seg_max.stride(0) if seg_max is not None else 4


def edge_seam_fwd(Pb, P0, pt, lnw_b, lnb_b, eps_b, Wp, bp, Sp, Sv, Sg, scale, Pout, ln_w, ln_b, eps, Wpt, bpt, Wc, bc,
                  XLp, pos, XR, att, bias, slope, plan_items, n_items, finalize, out, seg_max, seg_sum, part):
    """Block b's edge epilogue (P' = Pout) + block b+1's prologue and camera attention forward in one
    pass (csrc/edge_seam.hip edge_seam_fwd_kernel); outputs as edge_cam_fwd's plus Pout."""
    _req(Pb, "Pb", 32)
    ldXR = _rows32(XR, "XR")
    ldSv = _rows32(Sv, "Sv")
    st = lib().gasfm_edge_seam_fwd(_p(Pb), _p(P0), _p(pt), _p(lnw_b), _p(lnb_b), eps_b, _p(Wp), Wp.stride(0), _p(bp),
                                   _p(Sp), _p(Sv), ldSv, _p(Sg), scale, _p(Pout), _p(ln_w), _p(ln_b), eps, _p(Wpt),
                                   _p(bpt), _p(Wc), _p(bc), _p(XLp), XLp.stride(0), _p(pos), _p(XR), ldXR, _p(att),
                                   _p(bias), slope, _p(plan_items), n_items, int(finalize), _p(out),
                                   out.stride(0) if out is not None else 0, _p(seg_max), _p(seg_sum), _ld_stat(seg_max),
                                   _p(part), _stream(Pb))
    check(st, "gasfm_edge_seam_fwd")


def edge0_seam_fwd(P, pt, lna_w, lna_b, lnb_w, lnb_b, eps0, Wp, bp, Wsk, bsk, Sp, Sv, Sg, scale, Pout, ln_w, ln_b, eps,
                   Wpt, bpt, Wc, bc, XLp, pos, XR, att, bias, slope, plan_items, n_items, finalize, out, seg_max,
                   seg_sum, part):
    """Block 0's edge epilogue (2-wide P, edge0_epilogue_fwd) + block 1's prologue and camera
    attention forward in one pass (csrc/edge_seam.hip edge_seam_fwd_kernel, EP0); outputs as
    edge_seam_fwd's."""
    _req(P, "P", 2)
    ldXR = _rows32(XR, "XR")
    ldSv = _rows32(Sv, "Sv")
    st = lib().gasfm_edge0_seam_fwd(_p(P), _p(pt), _p(lna_w), _p(lna_b), _p(lnb_w), _p(lnb_b), eps0, _p(Wp), _p(bp),
                                    _p(Wsk), _p(bsk), _p(Sp), _p(Sv), ldSv, _p(Sg), scale, _p(Pout), _p(ln_w), _p(ln_b),
                                    eps, _p(Wpt), _p(bpt), _p(Wc), _p(bc), _p(XLp), XLp.stride(0), _p(pos), _p(XR),
                                    ldXR, _p(att), _p(bias), slope, _p(plan_items), n_items, int(finalize), _p(out),
                                    out.stride(0) if out is not None else 0, _p(seg_max), _p(seg_sum),
                                    _ld_stat(seg_max), _p(part), _stream(P))
    check(st, "gasfm_edge0_seam_fwd")


def edge_cam_pbwd_part_shape(n_items, dwp_cols=0):
    """(rows, cols) of edge_cam_pbwd's part buffer; dwp_cols = 32 or 34 with the dWp block (dwp)."""
    L = lib()
    return int(L.gasfm_edge_cam_pbwd_part_rows(n_items)), int(L.gasfm_edge_cam_pbwd_part_cols()) + 32 * dwp_cols


def edge_cam_pbwd(P, ln_w, ln_b, eps, Wpt, Wc, bc, Wp, scale, XR, att, bias, slope, out, seg_max, seg_sum, gout,
                  plan_items, n_items, dXLp, dRes, dP, dXR, part_dxr, part, ldStat=4, epi=None, dwp=None):
    """The camera attention's backward and the block's edge prologue backward in one pass
    (csrc/edge_cam.hip edge_cam_pbwd): dP, dXR (+ split partials), part rows
    [dW 64x32 | db 64 | dgamma 32 | dbeta 32 | datt 32 | 0 (32)] per workgroup (the attention bias
    gradient is the caller's column sum of gout).

    epi = (We, scale_e, dSv, part_dsv, dP0 or None): also the previous block's edge-epilogue
    gradients from this dP (dSv rows / split-camera partial rows of the same plan, dP0).
    dwp = P0 or None (requires ln_w and dRes): also this block's lin_proj weight gradient,
    [32 x (32 | 34)] appended to each part row (part has edge_cam_pbwd_part_shape(n, dwp=...) columns)."""
    _req(P, "P", 32)
    ldXR = _rows32(XR, "XR")
    We = dSv = part_dsv = dP0 = None
    scale_e, ldWe = 0.0, 0
    if epi is not None:
        We, scale_e, dSv, part_dsv, dP0 = epi
        _req(dSv, "dSv", 32)
        if dP0 is not None:
            _req(dP0, "dP0", 2)
        ldWe = We.stride(0)
    P0, ldWpo = None, 0
    if dwp is not False and dwp is not None:
        P0 = dwp if isinstance(dwp, torch.Tensor) else None
        ldWpo = 34 if P0 is not None else 32
    if P0 is not None:
        _req(P0, "P0", 2)
    st = lib().gasfm_edge_cam_pbwd_ex(_p(P), _p(ln_w), _p(ln_b), eps, _p(Wpt), _p(Wc), _p(bc), _p(Wp),
                                      Wp.stride(0) if Wp is not None else 0, scale, _p(XR), ldXR, _p(att), _p(bias),
                                      slope, _p(out), out.stride(0), _p(seg_max), _p(seg_sum), ldStat, _p(gout),
                                      gout.stride(0), _p(plan_items), n_items, _p(dXLp), dXLp.stride(0), _p(dRes),
                                      _p(dP), _p(dXR), dXR.stride(0), _p(part_dxr), _p(part), part.stride(0), _p(We),
                                      ldWe, scale_e, _p(dSv), _p(part_dsv), _p(dP0), _p(P0), ldWpo, _stream(P))
    check(st, "gasfm_edge_cam_pbwd")


def segment_rowsum(items, n_items, perm, X, scale, out, part):
    st = lib().gasfm_segment_rowsum(_p(items), n_items, _p(perm), _p(X), X.stride(0), scale, _p(out), _p(part),
                                    _stream(X))
    check(st, "gasfm_segment_rowsum")


# ---------------------------------------------------------------- set-of-set layer kernels
def sos_width_ok(d_in, d_out):
    return bool(lib().gasfm_sos_width_ok(int(d_in), int(d_out)))


def sos_row_tile(n_cols):
    return int(lib().gasfm_sos_row_tile(int(n_cols)))


def sos_segment_sum(plan, X, scale=1.0, mean=False, mask=None):
    """[num_targets, D] sums (means) of the rows of X over the plan's segments, optionally masked by
    mask > 0; split items go through partial rows and the plan's ordered combines."""
    _req(X, "sos_segment_sum X")
    D = X.shape[1]
    out = torch.zeros((plan.num_targets, D), dtype=torch.float32, device=X.device)
    if plan.n_items == 0 or X.shape[0] == 0:
        return out
    if mask is not None:
        _req(mask, "sos_segment_sum mask", D)
    part = torch.empty((plan.n_part_rows, D), dtype=torch.float32, device=X.device) if plan.n_part_rows else None
    st = lib().gasfm_sos_segment_sum(_p(plan.items), plan.n_items, _p(plan.perm), _p(X), X.stride(0), _p(mask),
                                     0 if mask is None else mask.stride(0), D, float(scale),
                                     _p(plan.seg_ptr) if mean else None, _p(out), _p(part), _stream(X))
    check(st, "gasfm_sos_segment_sum")
    if part is not None:
        if plan.n_l1:
            attn_bwd_combine(plan.combine_l1, plan.n_l1, D, part, part)
        if plan.n_combine:
            attn_bwd_combine(plan.combine, plan.n_combine, D, part, out)
    return out


def sos_edge_fwd(X, W, cam, pt, S, V, cmean, R, relu, out=None):
    _req(X, "sos_edge_fwd X")
    E, d_in = X.shape
    d_out = W.shape[0]
    for t, name, cols in ((W, "W", d_in), (S, "S", d_out), (V, "V", d_out)):
        _req(t, "sos_edge_fwd " + name, cols)
    Y = torch.empty((E, d_out), dtype=torch.float32, device=X.device) if out is None else out
    _req(Y, "sos_edge_fwd out", d_out)
    if Y.shape[0] != E:
        raise ValueError(f"sos_edge_fwd out: {Y.shape[0]} rows, expected {E}")
    if E == 0:
        return Y
    if cam.shape[0] != E or pt.shape[0] != E or cam.dtype != torch.int32 or pt.dtype != torch.int32:
        raise ValueError("sos_edge_fwd: cam / pt must be int32 [E]")
    if cmean is not None:
        _req(cmean, "sos_edge_fwd cmean", d_out)
    if R is not None:
        _req(R, "sos_edge_fwd R", d_out)
    st = lib().gasfm_sos_edge_fwd(_p(X), X.stride(0), _p(W), E, d_in, d_out, _p(cam), _p(pt), _p(S), _p(V),
                                  _p(cmean), _p(R), 0 if R is None else R.stride(0), int(bool(relu)), _p(Y),
                                  _stream(X))
    check(st, "gasfm_sos_edge_fwd")
    return Y


def sos_edge_dx(dY, Ym, W, cam, pt, Ac, Bp, E, d_in, out=None):
    """dX [E, d_in]; dY None: the gathered rows Ac[cam] + Bp[pt] alone."""
    dev = cam.device
    dX = torch.empty((E, d_in), dtype=torch.float32, device=dev) if out is None else out
    _req(dX, "sos_edge_dx out", d_in)
    if dX.shape[0] != E or cam.shape[0] != E or pt.shape[0] != E or (dY is not None and dY.shape[0] != E):
        raise ValueError("sos_edge_dx: row counts differ")
    if E == 0:
        return dX
    d_out = 0 if dY is None else dY.shape[1]
    for t, name, cols in ((dY, "dY", None), (Ym, "Ym", d_out), (W, "W", d_in), (Ac, "Ac", d_in), (Bp, "Bp", d_in)):
        if t is not None:
            _req(t, "sos_edge_dx " + name, cols)
    st = lib().gasfm_sos_edge_dx(_p(dY), _p(Ym), _p(W), E, d_in, d_out, _p(cam), _p(pt), _p(Ac), _p(Bp), _p(dX),
                                 _stream(dX))
    check(st, "gasfm_sos_edge_dx")
    return dX


def sos_edge_dw(dY, Ym, X):
    """dW [d_out, d_in] = (mask . dY / 4)^T X: split-K partial matrices, then the ordered colsum."""
    _req(dY, "sos_edge_dw dY")
    _req(X, "sos_edge_dw X")
    E, d_out = dY.shape
    d_in = X.shape[1]
    if E == 0:
        return torch.zeros((d_out, d_in), dtype=torch.float32, device=dY.device)
    if Ym is not None:
        _req(Ym, "sos_edge_dw Ym", d_out)
    L = lib()
    splits = int(L.gasfm_sos_dw_splits(E, d_in, d_out))
    part = torch.empty((splits, d_out * d_in), dtype=torch.float32, device=dY.device)
    st = L.gasfm_sos_edge_dw(_p(dY), _p(Ym), _p(X), X.stride(0), E, d_in, d_out, splits, _p(part), _stream(dY))
    check(st, "gasfm_sos_edge_dw")
    if splits == 1:
        return part.view(d_out, d_in)
    return colsum(part).view(d_out, d_in)


# ---------------------------------------------------------------- block 0 (2-wide) edge kernels
def edge0_part_rows(which, E, n_items=0):
    return lib().gasfm_edge0_part_rows(which, E, n_items)


def edge0_prologue_fwd(P, ln_w, ln_b, eps, W0, b0, XL, pos=None):
    _req(P, "P", 2)
    st = lib().gasfm_edge0_prologue_fwd(_p(P), P.shape[0], _p(ln_w), _p(ln_b), eps, _p(W0), _p(b0), _p(XL),
                                        _p(pos), _stream(P))
    check(st, "gasfm_edge0_prologue_fwd")


def edge0_prologue_fwd_rows(P, ln_w, ln_b, eps, W0, b0, XL, perm):
    _req(P, "P", 2)
    if perm.dtype != torch.int32 or perm.numel() != P.shape[0] or perm.device != P.device:
        raise ValueError("edge0_prologue_fwd_rows: perm must be int32 [E] on P's device")
    st = lib().gasfm_edge0_prologue_fwd_rows(_p(P), P.shape[0], _p(ln_w), _p(ln_b), eps, _p(W0), _p(b0), _p(XL),
                                             _p(perm), _stream(P))
    check(st, "gasfm_edge0_prologue_fwd_rows")


def edge0_epilogue_fwd(P, cam, pt, lna_w, lna_b, lnb_w, lnb_b, eps, Wp, bp, Wsk, bsk, Sp, Sv, Sg, scale, out):
    _req(P, "P", 2)
    for t, n in ((Sp, "Sp"), (Sg, "Sg")):
        _req(t, n)
    ldSv = _rows32(Sv, "Sv")
    st = lib().gasfm_edge0_epilogue_fwd(_p(P), _p(cam), _p(pt), P.shape[0], _p(lna_w), _p(lna_b), _p(lnb_w),
                                        _p(lnb_b), eps, _p(Wp), _p(bp), _p(Wsk), _p(bsk), _p(Sp), _p(Sv), ldSv,
                                        _p(Sg), scale, _p(out), _stream(P))
    check(st, "gasfm_edge0_epilogue_fwd")


def edge0_epilogue_bwd(items, n_items, dPo, P, lna_w, lna_b, lnb_w, lnb_b, eps, Wp, Wsk, scale, dSv, part_dsv, aux,
                       part):
    _req(dPo, "dP'", 32)
    st = lib().gasfm_edge0_epilogue_bwd(_p(items), n_items, _p(dPo), _p(P), _p(lna_w), _p(lna_b), _p(lnb_w),
                                        _p(lnb_b), eps, _p(Wp), _p(Wsk), scale, _p(dSv), _p(part_dsv), _p(aux),
                                        _p(part), _stream(dPo))
    check(st, "gasfm_edge0_epilogue_bwd")


def edge0_prologue_bwd(dXL, P, aux, ln_w, ln_b, eps, W0, dP, part):
    _req(dXL, "dXL0", 8)
    st = lib().gasfm_edge0_prologue_bwd(_p(dXL), _p(P), _p(aux), P.shape[0], _p(ln_w), _p(ln_b), eps, _p(W0),
                                        _p(dP), _p(part), _stream(P))
    check(st, "gasfm_edge0_prologue_bwd")


# ---------------------------------------------------------------- point-node LayerNorm -> ReLU -> Linear
def node_part_rows(N, n_out, residual):
    return lib().gasfm_node_part_rows(N, n_out, int(residual))


def node_ln_linear_fwd(X, ln_w, ln_b, eps, W, b, residual, Y):
    _req(X, "X")
    N, n_in = X.shape
    st = lib().gasfm_node_ln_linear_fwd(_p(X), N, n_in, _p(ln_w), _p(ln_b), eps, _p(W), _p(b), W.shape[0],
                                        int(residual), _p(Y), Y.stride(0), _stream(X))
    check(st, "gasfm_node_ln_linear_fwd")


def node_ln_linear_bwd(dY, X, ln_w, ln_b, eps, W, residual, dX, part):
    _req(dY, "dY", W.shape[0])
    _req(X, "X")
    N, n_in = X.shape
    st = lib().gasfm_node_ln_linear_bwd(_p(dY), _p(X), N, n_in, _p(ln_w), _p(ln_b), eps, _p(W), W.shape[0],
                                        int(residual), _p(dX), _p(part), _stream(X))
    check(st, "gasfm_node_ln_linear_bwd")


# ---------------------------------------------------------------- global node (one row)
def gvec_bwd_chunks(N):
    return lib().gasfm_gvec_bwd_chunks(N)


def gvec_fwd(x, ln_w, ln_b, eps, W, b, res, y):
    _req(x, "x")
    _req(W, "W")
    st = lib().gasfm_gvec_fwd(_p(x), W.shape[1], _p(ln_w), _p(ln_b), eps, _p(W), _p(b), W.shape[0], _p(res), _p(y),
                              _stream(x))
    check(st, "gasfm_gvec_fwd")


def gvec_bwd(dy, x, ln_w, ln_b, eps, W, resid, dx, dW, db, dgam, dbet, part):
    _req(dy, "dy")
    st = lib().gasfm_gvec_bwd(_p(dy), _p(x), W.shape[1], _p(ln_w), _p(ln_b), eps, _p(W), W.shape[0], int(resid),
                              _p(dx), _p(dW), _p(db), _p(dgam), _p(dbet), _p(part), _stream(x))
    check(st, "gasfm_gvec_bwd")


# ---------------------------------------------------------------- scene-point block chains (point_block.hip)
def point_tail_part_shape(N, has_prev):
    cols = ctypes.c_int32(0)
    rows = lib().gasfm_point_tail_part_shape(N, int(has_prev), ctypes.byref(cols))
    return rows, cols.value


def point_hub_part_shape(N, which, has_res):
    cols = ctypes.c_int32(0)
    rows = lib().gasfm_point_hub_part_shape(N, int(which), int(has_res), ctypes.byref(cols))
    return rows, cols.value


def point_tail_fwd(prev, agg, Wp, bp, ln_w, ln_b, eps, Wm, bm, out):
    _req(agg, "agg", 32)
    if prev is not None:
        _req(prev, "prev", 64)
    st = lib().gasfm_point_tail_fwd(_p(prev), _p(agg), agg.shape[0], _p(Wp), _p(bp), _p(ln_w), _p(ln_b), eps,
                                    _p(Wm), _p(bm), _p(out), _stream(agg))
    check(st, "gasfm_point_tail_fwd")


def point_tail_bwd(dout, prev, agg, Wp, bp, ln_w, ln_b, eps, Wm, dx, dagg, part):
    _req(dout, "dout", 64)
    _req(agg, "agg", 32)
    if prev is not None:
        _req(prev, "prev", 64)
    st = lib().gasfm_point_tail_bwd(_p(dout), _p(prev), _p(agg), agg.shape[0], _p(Wp), _p(bp), _p(ln_w), _p(ln_b),
                                    eps, _p(Wm), _p(dx), _p(dagg), _p(part), _stream(agg))
    check(st, "gasfm_point_tail_bwd")


def point_hub_fwd(X, eps, gA, bA, WA, SA, WB, bB, XL, gC, bC, WC, bWC, WD, bD, XR):
    _req(X, "X", 64)
    st = lib().gasfm_point_hub_fwd(_p(X), X.shape[0], eps, _p(gA), _p(bA), _p(WA), _p(SA), _p(WB), _p(bB), _p(XL),
                                   _p(gC), _p(bC), _p(WC), _p(bWC), _p(WD), _p(bD), _p(XR), _stream(X))
    check(st, "gasfm_point_hub_fwd")


def point_tail_hub_fwd(prev, agg, Wp, bp, ln_w, ln_b, eps, Wm, bm, out, eps_h, gA, bA, WA, SA, WB, bB, XL, gC, bC,
                       WC, bWC, WD, bD, XR):
    """point_tail_fwd + point_hub_fwd on its output in one launch (out = p)."""
    _req(agg, "agg", 32)
    _req(out, "out", 64)
    if prev is not None:
        _req(prev, "prev", 64)
    st = lib().gasfm_point_tail_hub_fwd(_p(prev), _p(agg), agg.shape[0], _p(Wp), _p(bp), _p(ln_w), _p(ln_b), eps,
                                        _p(Wm), _p(bm), _p(out), eps_h, _p(gA), _p(bA), _p(WA), _p(SA), _p(WB), _p(bB),
                                        _p(XL), _p(gC), _p(bC), _p(WC), _p(bWC), _p(WD), _p(bD), _p(XR), _stream(agg))
    check(st, "gasfm_point_tail_hub_fwd")


def point_hub_bwd(X, eps, gA, bA, WA, WB, gC, bC, WC, bWC, WD, dSA, dXL, dXR, dRes, dX, part_a, part_c):
    """The whole point-hub backward in one pass (gasfm_point_hub_bwd)."""
    _req(X, "X", 64)
    _req(dSA, "dSA", 32)
    _req(dXL, "dXL", 64)
    _req(dXR, "dXR", 32)
    if dRes is not None:
        _req(dRes, "dRes", 64)
    st = lib().gasfm_point_hub_bwd(_p(X), X.shape[0], eps, _p(gA), _p(bA), _p(WA), _p(WB), _p(gC), _p(bC), _p(WC),
                                   _p(bWC), _p(WD), _p(dSA), _p(dXL), _p(dXR), _p(dRes), _p(dX), _p(part_a),
                                   _p(part_c), _stream(X))
    check(st, "gasfm_point_hub_bwd")


# ---------------------------------------------------------------- input embedding (embed.hip)
def embed2_fwd(X, W, b, Y):
    _req(X, "values", 2)
    _req(Y, "P", 2)
    st = lib().gasfm_embed2_fwd(_p(X), X.shape[0], _p(W), _p(b), _p(Y), _stream(X))
    check(st, "gasfm_embed2_fwd")


def embed2_bwd(X, dY, defer=False):
    """(dW [2, 2], db [2]) of P = X W^T + b from dP; column sums through param_colsum."""
    _req(X, "values", 2)
    _req(dY, "dP", 2)
    E = X.shape[0]
    rows = lib().gasfm_embed2_part_rows(E)
    if rows == 0:
        tot = torch.zeros(6, dtype=torch.float32, device=X.device)
    else:
        part = torch.empty((rows, 6), dtype=torch.float32, device=X.device)
        st = lib().gasfm_embed2_bwd(_p(X), _p(dY), E, _p(part), _stream(X))
        check(st, "gasfm_embed2_bwd")
        tot = param_colsum(part, defer)
    return tot[:4].view(2, 2), tot[4:]


# ---------------------------------------------------------------- scene-point head (point_head.hip)
def point_head_part_shape(N, which):
    cols = ctypes.c_int32(0)
    rows = lib().gasfm_point_head_part_shape(N, int(which), ctypes.byref(cols))
    return rows, cols.value


def _head_weights(W1, b1, W2, b2, W3, b3=None):
    shapes = ((W1, (64, 64)), (b1, (64,)), (W2, (64, 64)), (b2, (64,)), (W3, (3, 64))) + \
        (((b3, (3,)),) if b3 is not None else ())
    for t, shape in shapes:
        if tuple(t.shape) != shape or not t.is_contiguous() or t.dtype != torch.float32:
            raise ValueError(f"point head: weight {tuple(t.shape)} is not a contiguous fp32 {shape}")


def point_head_fwd(P, W1, b1, W2, b2, W3, b3, out):
    _req(P, "P", 64)
    _head_weights(W1, b1, W2, b2, W3, b3)
    N = P.shape[0]
    if tuple(out.shape) != (4, N) or not out.is_contiguous():
        raise ValueError("point_head_fwd: out must be a contiguous [4, N]")
    st = lib().gasfm_point_head_fwd(_p(P), N, _p(W1), _p(b1), _p(W2), _p(b2), _p(W3), _p(b3), _p(out), _stream(P))
    check(st, "gasfm_point_head_fwd")


def point_head_bwd(P, W1, b1, W2, b2, W3, dout, dP, part_a, part_b):
    _req(P, "P", 64)
    _req(dP, "dP", 64)
    _head_weights(W1, b1, W2, b2, W3)
    N = P.shape[0]
    if tuple(dout.shape) != (4, N) or not dout.is_contiguous():
        raise ValueError("point_head_bwd: dout must be a contiguous [4, N]")
    for part, which in ((part_a, 0), (part_b, 1)):
        if tuple(part.shape) != point_head_part_shape(N, which) or not part.is_contiguous():
            raise ValueError("point_head_bwd: partial buffer of the wrong shape")
    st = lib().gasfm_point_head_bwd(_p(P), N, _p(W1), _p(b1), _p(W2), _p(b2), _p(W3), _p(dout), _p(dP),
                                    _p(part_a), _p(part_b), _stream(P))
    check(st, "gasfm_point_head_bwd")


# ---------------------------------------------------------------- camera-side block chains (view_block.hip)
def view_tail_part_cols(D):
    return lib().gasfm_view_tail_part_cols(D)


def view_hub_part_cols(D):
    return lib().gasfm_view_hub_part_cols(D)


def view_scratch(m, D, device):
    return torch.empty(max(1, int(lib().gasfm_view_scratch_floats(m, D))), dtype=torch.float32, device=device)


def view_tail_fwd(prev, agg, Wp, bp, ln_w, ln_b, eps, bm, x, xb, h, rs, scratch):
    _req(agg, "agg", 32)
    D = x.shape[1]
    if prev is not None:
        _req(prev, "prev", D)
    st = lib().gasfm_view_tail_fwd(_p(prev), _p(agg), agg.shape[0], D, _p(Wp), _p(bp), _p(ln_w), _p(ln_b), eps,
                                   _p(bm), _p(x), _p(xb), _p(h), _p(rs), _p(scratch), _stream(agg))
    check(st, "gasfm_view_tail_fwd")


def view_tail_bwd(dv, dh, x, rs, agg, Wp, ln_w, ln_b, dx, dagg, part, scratch):
    D = x.shape[1]
    for t, n in ((dv, "dv"), (dh, "dh"), (x, "x")):
        _req(t, n, D)
    _req(agg, "agg", 32)
    st = lib().gasfm_view_tail_bwd(_p(dv), _p(dh), _p(x), _p(rs), _p(agg), agg.shape[0], D, _p(Wp), _p(ln_w),
                                   _p(ln_b), _p(dx), _p(dagg), _p(part), _p(scratch), _stream(agg))
    check(st, "gasfm_view_tail_bwd")


def view_hub_fwd(v, eps, gC, bC, Wv, gA, bA, Wa, ba, Wr, br, sv, t, xr, rs, scratch):
    """sv / xr: [m, 32] with a common row stride (two column halves of one [m, 64] block, or two
    contiguous tensors)."""
    _req(v, "v")
    ldo = _rows32(sv, "sv")
    if _rows32(xr, "xr") != ldo:
        raise ValueError("view_hub_fwd: sv and xr need the same row stride")
    st = lib().gasfm_view_hub_fwd(_p(v), v.shape[0], v.shape[1], eps, _p(gC), _p(bC), _p(Wv), _p(gA), _p(bA), _p(Wa),
                                  _p(ba), _p(Wr), _p(br), _p(sv), _p(t), _p(xr), ldo, _p(rs), _p(scratch), _stream(v))
    check(st, "gasfm_view_hub_fwd")


def view_chain_ok(m, D):
    return bool(lib().gasfm_view_chain_ok(m, D))


def _vc_scratch(m, D, device):
    return torch.empty(max(1, int(lib().gasfm_view_chain_scratch_floats(m, D))), dtype=torch.float32, device=device)


def view_chain_tail_fwd(prev, agg, Wp, bp, ln_w, ln_b, eps, Wm, bm, view, x, h, rs):
    _req(agg, "agg", 32)
    m, D = view.shape
    for t, n in ((view, "view"), (x, "x"), (h, "h"), (Wm, "Wm"), (Wp, "Wp")) + (((prev, "prev"),) if prev is not None else ()):
        _req(t, n)
    st = lib().gasfm_view_chain_tail_fwd(_p(prev), _p(agg), m, D, _p(Wp), _p(bp), _p(ln_w), _p(ln_b), eps, _p(Wm),
                                         _p(bm), _p(view), _p(x), _p(h), _p(rs), _stream(agg))
    check(st, "gasfm_view_chain_tail_fwd")


def view_chain_hub_fwd(v, eps, Wl, bl, gC, bC, Wv, gA, bA, Wa, ba, Wr, br, XL, sv, t, xr, rs):
    _req(v, "v")
    ldo = _rows32(sv, "sv")
    if _rows32(xr, "xr") != ldo:
        raise ValueError("view_chain_hub_fwd: sv and xr need the same row stride")
    for a, n in ((Wl, "Wl"), (Wv, "Wv"), (Wa, "Wa"), (XL, "XL")):
        _req(a, n)
    st = lib().gasfm_view_chain_hub_fwd(_p(v), v.shape[0], v.shape[1], eps, _p(Wl), _p(bl), _p(gC), _p(bC), _p(Wv),
                                        _p(gA), _p(bA), _p(Wa), _p(ba), _p(Wr), _p(br), _p(XL), _p(sv), _p(t), _p(xr),
                                        ldo, _p(rs), _stream(v))
    check(st, "gasfm_view_chain_hub_fwd")


def view_chain_hub_bwd(v, rs, gC, bC, Wv, gA, bA, Wa, t, Wr, Wl, dsv, dxr, dxl, dres, dacc, dWl, part):
    _req(v, "v")
    m, D = v.shape
    for a, n, w in ((t, "t", 32), (dsv, "dsv", 32), (dxr, "dxr", 32), (dxl, "dxl", D), (dacc, "dacc", D),
                    (dWl, "dWl", D)):
        _req(a, n, w)
    if dres is not None:
        _req(dres, "dres", D)
    scratch = _vc_scratch(m, D, v.device)
    st = lib().gasfm_view_chain_hub_bwd(_p(v), _p(rs), m, D, _p(gC), _p(bC), _p(Wv), _p(gA), _p(bA), _p(Wa), _p(t),
                                        _p(Wr), _p(Wl), _p(dsv), _p(dxr), _p(dxl), _p(dres), _p(dacc), _p(dWl),
                                        _p(part), _p(scratch), _stream(v))
    check(st, "gasfm_view_chain_hub_bwd")


def view_chain_tail_bwd(dv, x, h, rs, agg, Wp, ln_w, ln_b, Wm, dh, dWm, dx, dagg, part):
    m, D = x.shape
    for a, n in ((dv, "dv"), (x, "x"), (h, "h"), (dh, "dh"), (dx, "dx"), (dWm, "dWm")):
        _req(a, n, D)
    _req(agg, "agg", 32)
    scratch = _vc_scratch(m, D, x.device)
    cnt = _counters(x.device, lib().gasfm_view_chain_counters(m))
    st = lib().gasfm_view_chain_tail_bwd(_p(dv), _p(x), _p(h), _p(rs), _p(agg), m, D, _p(Wp), _p(ln_w), _p(ln_b),
                                         _p(Wm), _p(dh), _p(dWm), _p(dx), _p(dagg), _p(part), _p(scratch), _p(cnt),
                                         _stream(x))
    check(st, "gasfm_view_chain_tail_bwd")


def view_hub_bwd(v, rs, gC, bC, Wv, gA, bA, Wa, t, Wr, dsv, dxr, dxl, dacc, part, scratch, dres=None):
    """dres (d skip, or None) is added to dacc in the kernel's second pass."""
    _req(v, "v")
    D = v.shape[1]
    for a, n, w in ((t, "t", 32), (dsv, "dsv", 32), (dxr, "dxr", 32), (dxl, "dxl", D), (dacc, "dacc", D)):
        _req(a, n, w)
    if dres is not None:
        _req(dres, "dres", D)
    st = lib().gasfm_view_hub_bwd(_p(v), _p(rs), v.shape[0], D, _p(gC), _p(bC), _p(Wv), _p(gA), _p(bA), _p(Wa),
                                  _p(t), _p(Wr), _p(dsv), _p(dxr), _p(dxl), _p(dres), _p(dacc), _p(part),
                                  _p(scratch), _stream(v))
    check(st, "gasfm_view_hub_bwd")


# ---------------------------------------------------------------- calibrated camera head (pose_head.hip)
def pose_fwd(x, P):
    if not x.is_cuda or x.dtype != torch.float32 or x.stride(1) != 1:
        raise TypeError("pose x: expected a float32 CUDA tensor with unit column stride (no CPU fallback)")
    check(lib().gasfm_pose_fwd(_p(x), x.stride(0), x.shape[0], _p(P), _stream(x)), "gasfm_pose_fwd")


def pose_bwd(x, dP, dx):
    _req(dP, "dP")
    check(lib().gasfm_pose_bwd(_p(x), x.stride(0), x.shape[0], _p(dP), _p(dx), dx.stride(0), _stream(x)),
          "gasfm_pose_bwd")


# ------------------- per-edge losses and metrics (edge_loss.hpp: esfm_loss.hip, ose_loss.hip)
def _i32vec(t, name):
    if not t.is_cuda or t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous():
        raise TypeError(f"{name}: expected a contiguous int32 CUDA vector")


def _edge_args(name, cam, pt, vals, P, X, csr=None, seg=None, scene_of=None, f32=()):
    """Validate the argument family of the per-edge kernels and return (E, m, n): int32 vectors cam /
    pt [E], vals [E, 2], P [m, 12], X [4, n]; ``csr`` = (cam_ptr [m + 1], pt_ptr [n + 1], perm [E] or
    None); ``seg`` = (eoff [S + 1], S); ``scene_of`` = the (camera [m], point [n]) scene maps; ``f32`` =
    further (tensor, name, columns or None) float32 operands."""
    vecs = [(cam, "cam"), (pt, "pt")]
    if csr is not None:
        vecs += [(csr[0], "cam_ptr"), (csr[1], "pt_ptr")] + ([] if csr[2] is None else [(csr[2], "perm")])
    if scene_of is not None:
        vecs += [(scene_of[0], "scene_of_cam"), (scene_of[1], "scene_of_pt")]
    for t, tname in vecs:
        _i32vec(t, f"{name}: {tname}")
    for t, tname, cols in ((vals, "vals", 2), (P, "P", 12), (X, "pts3D", None)) + tuple(f32):
        _req(t, f"{name}: {tname}", cols)
    if X.dim() != 2 or X.shape[0] != 4 or P.dim() != 2 or vals.dim() != 2:
        raise ValueError(f"{name}: expected P [m, 12], pts3D [4, n] and vals [E, 2]")
    E, m, n = cam.shape[0], P.shape[0], X.shape[1]
    if pt.shape[0] != E or vals.shape[0] != E:
        raise ValueError(f"{name}: expected pts3D [4, n] and E-long cam / pt / values")
    if csr is not None and (csr[0].shape[0] != m + 1 or csr[1].shape[0] != n + 1
                            or (csr[2] is not None and csr[2].shape[0] != E)):
        raise ValueError(f"{name}: CSR shapes do not match m / n / E")
    if scene_of is not None and (scene_of[0].shape[0] != m or scene_of[1].shape[0] != n):
        raise ValueError(f"{name}: scene map shapes do not match m / n")
    if seg is not None:
        eoff, S = seg
        if not eoff.is_cuda or eoff.dtype != torch.int32 or not eoff.is_contiguous() or eoff.numel() != S + 1:
            raise TypeError(f"{name}: eoff must be a contiguous int32 [S + 1] CUDA tensor")
    return E, m, n


def _grad_args(dloss, dP, dX, n, tot=None):
    return ((dloss, "dloss", None), (dP, "dP", 12), (dX, "dX", n)) + (() if tot is None else ((tot, "tot", None),))


def esfm_part_rows(E):
    return lib().gasfm_esfm_part_rows(E)


def esfm_fwd(cam, pt, vals, P, X, margin, hinge_w, hinge, part):
    E, _, n = _edge_args("esfm_fwd", cam, pt, vals, P, X)
    st = lib().gasfm_esfm_fwd(_p(cam), _p(pt), _p(vals), E, _p(P), _p(X), n, margin, hinge_w, int(hinge), _p(part),
                              _stream(X))
    check(st, "gasfm_esfm_fwd")


def esfm_bwd(cptr, pptr, perm, cam, pt, vals, P, X, margin, hinge_w, hinge, equalize, valid_only, dloss, tot, dP,
             dX, E_norm=None):
    """E_norm: the edge count of the mean (default the local E; the global count on a sharded scene)."""
    E, m, n = _edge_args("esfm_bwd", cam, pt, vals, P, X, csr=(cptr, pptr, perm),
                         f32=_grad_args(dloss, dP, dX, X.shape[-1], tot))
    E_norm = E if E_norm is None else int(E_norm)
    st = lib().gasfm_esfm_bwd(_p(cptr), m, _p(pptr), _p(perm), _p(cam), _p(pt), _p(vals), E, E_norm, _p(P), _p(X), n,
                              margin, hinge_w, int(hinge), int(equalize), int(valid_only), _p(dloss), _p(tot), _p(dP),
                              _p(dX), _stream(X))
    check(st, "gasfm_esfm_bwd")


def esfm_seg_fwd(cam, pt, vals, eoff, weight, P, X, margin, hinge_w, hinge):
    """Union-batch ESFMLoss forward (gasfm_esfm_seg_fwd): (loss [1], tot [S, 2])."""
    S = int(weight.numel())
    _, _, n = _edge_args("esfm_seg_fwd", cam, pt, vals, P, X, seg=(eoff, S), f32=((weight, "weight", None),))
    dev = X.device
    part = torch.empty((lib().gasfm_esfm_seg_part_rows(S), 2), dtype=torch.float32, device=dev)
    tot = torch.empty((S, 2), dtype=torch.float32, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    st = lib().gasfm_esfm_seg_fwd(_p(cam), _p(pt), _p(vals), _p(eoff), S, _p(weight), _p(P), _p(X), n, margin, hinge_w,
                                  int(hinge), _p(part), _p(tot), _p(loss), _stream(X))
    check(st, "gasfm_esfm_seg_fwd")
    return loss, tot


def esfm_seg_bwd(cptr, pptr, perm, cam, pt, vals, eoff, scene_of_cam, scene_of_pt, weight, P, X, margin, hinge_w,
                 hinge, equalize, valid_only, dloss, tot, dP, dX):
    """Union-batch ESFMLoss backward (gasfm_esfm_seg_bwd) into dP [m, 12] and dX [4, n]."""
    S = int(weight.numel())
    _, m, n = _edge_args("esfm_seg_bwd", cam, pt, vals, P, X, csr=(cptr, pptr, perm), seg=(eoff, S),
                         scene_of=(scene_of_cam, scene_of_pt),
                         f32=((weight, "weight", None),) + _grad_args(dloss, dP, dX, X.shape[-1], tot))
    st = lib().gasfm_esfm_seg_bwd(_p(cptr), m, _p(pptr), _p(perm), _p(cam), _p(pt), _p(vals), _p(eoff), S,
                                  _p(scene_of_cam), _p(scene_of_pt), _p(weight), _p(P), _p(X), n, margin, hinge_w,
                                  int(hinge), int(equalize), int(valid_only), _p(dloss), _p(tot), _p(dP), _p(dX),
                                  _stream(X))
    check(st, "gasfm_esfm_seg_bwd")


def ose_fwd(cam, pt, vals, P, X, w_reg):
    """Per-workgroup sums [rows, 1] of the OSE + exp-depth terms (finish with colsum)."""
    E, _, n = _edge_args("ose_fwd", cam, pt, vals, P, X)
    part = torch.empty((lib().gasfm_ose_part_rows(E), 1), dtype=torch.float32, device=X.device)
    st = lib().gasfm_ose_fwd(_p(cam), _p(pt), _p(vals), E, _p(P), _p(X), n, w_reg, _p(part), _stream(X))
    check(st, "gasfm_ose_fwd")
    return part


def ose_bwd(cptr, pptr, perm, cam, pt, vals, P, X, w_reg, dloss, dP, dX):
    E, m, n = _edge_args("ose_bwd", cam, pt, vals, P, X, csr=(cptr, pptr, perm),
                         f32=_grad_args(dloss, dP, dX, X.shape[-1]))
    st = lib().gasfm_ose_bwd(_p(cptr), m, _p(pptr), _p(perm), _p(cam), _p(pt), _p(vals), E, _p(P), _p(X), n, w_reg,
                             _p(dloss), _p(dP), _p(dX), _stream(X))
    check(st, "gasfm_ose_bwd")


def ose_seg_fwd(cam, pt, vals, eoff, weight, P, X, w_reg):
    """Union-batch OSE loss forward (gasfm_ose_seg_fwd): (loss [1], tot [S])."""
    S = int(weight.numel())
    _, _, n = _edge_args("ose_seg_fwd", cam, pt, vals, P, X, seg=(eoff, S), f32=((weight, "weight", None),))
    dev = X.device
    part = torch.empty(lib().gasfm_ose_seg_part_rows(S), dtype=torch.float32, device=dev)
    tot = torch.empty(S, dtype=torch.float32, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    st = lib().gasfm_ose_seg_fwd(_p(cam), _p(pt), _p(vals), _p(eoff), S, _p(weight), _p(P), _p(X), n, w_reg, _p(part),
                                 _p(tot), _p(loss), _stream(X))
    check(st, "gasfm_ose_seg_fwd")
    return loss, tot


def ose_seg_bwd(cptr, pptr, perm, cam, pt, vals, eoff, scene_of_cam, scene_of_pt, weight, P, X, w_reg, dloss, dP, dX):
    """Union-batch OSE loss backward (gasfm_ose_seg_bwd) into dP [m, 12] and dX [4, n]."""
    S = int(weight.numel())
    _, m, n = _edge_args("ose_seg_bwd", cam, pt, vals, P, X, csr=(cptr, pptr, perm), seg=(eoff, S),
                         scene_of=(scene_of_cam, scene_of_pt),
                         f32=((weight, "weight", None),) + _grad_args(dloss, dP, dX, X.shape[-1]))
    st = lib().gasfm_ose_seg_bwd(_p(cptr), m, _p(pptr), _p(perm), _p(cam), _p(pt), _p(vals), _p(eoff), S,
                                 _p(scene_of_cam), _p(scene_of_pt), _p(weight), _p(P), _p(X), n, w_reg, _p(dloss),
                                 _p(dP), _p(dX), _stream(X))
    check(st, "gasfm_ose_seg_bwd")


def reproj_error(cam, pt, xy, P, X, err=None):
    """Per-workgroup (sum, count) of the non-NaN reprojection errors (and err[e] if given)."""
    E, _, n = _edge_args("reproj_error", cam, pt, xy, P, X, f32=() if err is None else ((err, "err", None),))
    if err is not None and err.shape[0] != E:
        raise ValueError("reproj_error: expected pts3D [4, n] and E-long cam / pt / xy / err")
    part = torch.empty((esfm_part_rows(E), 2), dtype=torch.float32, device=X.device)
    st = lib().gasfm_reproj_error(_p(cam), _p(pt), _p(xy), E, _p(P), _p(X), n, _p(err), _p(part), _stream(X))
    check(st, "gasfm_reproj_error")
    return part


def reproj_error_seg(cam, pt, xy, eoff, S, P, X):
    """Per scene of a union batch: tot [S, 2] = (sum of the non-NaN reprojection errors, count)."""
    _, _, n = _edge_args("reproj_error_seg", cam, pt, xy, P, X, seg=(eoff, S))
    dev = X.device
    part = torch.empty((lib().gasfm_esfm_seg_part_rows(S), 2), dtype=torch.float32, device=dev)
    tot = torch.empty((S, 2), dtype=torch.float32, device=dev)
    st = lib().gasfm_reproj_error_seg(_p(cam), _p(pt), _p(xy), _p(eoff), S, _p(P), _p(X), n, _p(part), _p(tot),
                                      _stream(X))
    check(st, "gasfm_reproj_error_seg")
    return tot


def depth_stats(cam, pt, cam_ptr, pt_ptr, perm, P, X, margin, depth=None):
    """gasfm_depth_stats: (cam_neg [m] int32, pt_neg [n] int32, stats [6] float64 = #negative edges,
    #cameras / #points with an edge, sum, min, max of the edge depths); ``depth`` ([E] float32) is
    filled when given.  ``perm`` None = the point CSR covers the edges in their own order."""
    E, m, n = cam.shape[0], cam_ptr.shape[0] - 1, pt_ptr.shape[0] - 1
    for t, name in ((cam, "cam"), (pt, "pt"), (cam_ptr, "cam_ptr"), (pt_ptr, "pt_ptr")):
        _i32vec(t, name)
    if perm is not None:
        _i32vec(perm, "perm")
    _req(P, "P", 12), _req(X, "pts3D", n)
    if (X.dim() != 2 or X.shape[0] != 4 or P.dim() != 2 or P.shape[0] != m or pt.shape[0] != E
            or (perm is not None and perm.shape[0] != E) or (depth is not None and depth.shape[0] != E)):
        raise ValueError("depth_stats: expected P [m, 12], pts3D [4, n], cam_ptr [m + 1], pt_ptr [n + 1] and "
                         "E-long cam / pt / perm / depth")
    if depth is not None:
        _req(depth, "depth")
    dev = cam_ptr.device
    cam_neg = torch.empty(m, dtype=torch.int32, device=dev)
    pt_neg = torch.empty(n, dtype=torch.int32, device=dev)
    stats = torch.empty(6, dtype=torch.float64, device=dev)
    L = lib()
    ws = torch.empty(int(L.gasfm_depth_stats_ws_doubles(E)), dtype=torch.float64, device=dev)
    st = L.gasfm_depth_stats(_p(cam), _p(pt), E, _p(cam_ptr), m, _p(pt_ptr), _p(perm), n, _p(P), _p(X),
                             float(margin), _p(depth), _p(cam_neg), _p(pt_neg), _p(ws), _p(stats), _stream(cam_ptr))
    check(st, "gasfm_depth_stats")
    return cam_neg, pt_neg, stats


# ------------------------------------------- DirectDepthLoss (depth_loss.hip)
def _depth_args(a, b, name):
    _req(a, "depths"), _req(b, "depth targets")
    if a.dim() != 1 or a.shape != b.shape or a.shape[0] == 0:
        raise ValueError(f"{name}: expected two non-empty [E] vectors, got {tuple(a.shape)}, {tuple(b.shape)}")


def depth_loss_fwd(a, b, l2):
    """(sums [2] = (sum a, sum b), tot [2] = (sum of terms, sum of g_e a_e)) of DirectDepthLoss."""
    _depth_args(a, b, "depth_loss_fwd")
    E, L = a.shape[0], lib()
    part = torch.empty((L.gasfm_depth_loss_part_rows(E), 2), dtype=torch.float32, device=a.device)
    check(L.gasfm_depth_loss_sums(_p(a), _p(b), E, _p(part), _stream(a)), "gasfm_depth_loss_sums")
    sums = colsum(part)
    part = torch.empty_like(part)
    check(L.gasfm_depth_loss_fwd(_p(a), _p(b), E, _p(sums), int(l2), _p(part), _stream(a)), "gasfm_depth_loss_fwd")
    return sums, colsum(part)


def depth_loss_bwd(a, b, sums, tot, l2, dloss):
    _depth_args(a, b, "depth_loss_bwd")
    _req(dloss, "dloss")
    da = torch.empty_like(a)
    st = lib().gasfm_depth_loss_bwd(_p(a), _p(b), a.shape[0], _p(sums), _p(tot), int(l2), _p(dloss), _p(da),
                                    _stream(a))
    check(st, "gasfm_depth_loss_bwd")
    return da


UnionScene = _abi.structs["gasfm_union_scene"]
UnionOut = _abi.structs["gasfm_union_out"]
UnionPad = _abi.structs["gasfm_union_pad"]


def union_fill_scene(sc, out, stream_of):
    check(lib().gasfm_union_fill_scene(ctypes.byref(sc), ctypes.byref(out), _stream(stream_of)),
          "gasfm_union_fill_scene")


def fold_scene_rows_fwd(sv, sg, soc):
    """sv [m, w] + sg[soc] (gasfm_fold_scene_rows_fwd); unit column strides."""
    out = torch.empty((sv.shape[0], sv.shape[1]), dtype=torch.float32, device=sv.device)
    check(lib().gasfm_fold_scene_rows_fwd(_p(sv), sv.stride(0), _p(sg), sg.stride(0), _p(soc), sv.shape[0],
                                          sv.shape[1], _p(out), out.stride(0), _stream(sv)), "gasfm_fold_scene_rows_fwd")
    return out


def fold_scene_rows_bwd(dout, soc, S):
    """[S, w] per-scene sums of dout's rows in camera order (gasfm_fold_scene_rows_bwd)."""
    dsg = torch.empty((S, dout.shape[1]), dtype=torch.float32, device=dout.device)
    check(lib().gasfm_fold_scene_rows_bwd(_p(dout), dout.stride(0), _p(soc), dout.shape[0], S, dout.shape[1], _p(dsg),
                                          dsg.stride(0), _stream(dout)), "gasfm_fold_scene_rows_bwd")
    return dsg


ADAM_CHUNK = _C["GASFM_ADAM_CHUNK"]


def adam_step(tensors, chunks, n_chunks, lr, beta1, beta2, eps, weight_decay, step, stream_of):
    """gasfm_adam_step over device tables (uint8 tensors holding gasfm_adam_tensor / _chunk rows)."""
    check(lib().gasfm_adam_step(_p(tensors), _p(chunks), int(n_chunks), float(lr), float(beta1), float(beta2),
                                float(eps), float(weight_decay), int(step), _stream(stream_of)), "gasfm_adam_step")


CLIP_MODES = {None: _C["GASFM_CLIP_NONE"], "norm": _C["GASFM_CLIP_NORM"], "value": _C["GASFM_CLIP_VALUE"]}
# a gasfm_adam_ctl as fp32 words: int32 skip, then grad_norm, gscale, step_size, inv_bc2_sqrt
ADAM_CTL_FLOATS = ctypes.sizeof(_abi.structs["gasfm_adam_ctl"]) // 4


def grad_sumsq(tensors, chunks, n_chunks, partial, stream_of):
    """partial[i] (fp64) = the sum of squares of chunk i's gradient values (gasfm_grad_sumsq)."""
    check(lib().gasfm_grad_sumsq(_p(tensors), _p(chunks), int(n_chunks), _p(partial), _stream(stream_of)),
          "gasfm_grad_sumsq")


def grad_sumsq_finish(partial, n, total, norm):
    """total (fp64) = the first n partials in a fixed order, norm (fp32) = sqrt(total)."""
    check(lib().gasfm_grad_sumsq_finish(_p(partial), int(n), _p(total), _p(norm), _stream(total)),
          "gasfm_grad_sumsq_finish")


def grad_clip(tensors, chunks, n_chunks, mode, threshold, norm, stream_of):
    """In-place clip of the table's gradients: mode 'norm' (coefficient from the device norm) or 'value'."""
    check(lib().gasfm_grad_clip(_p(tensors), _p(chunks), int(n_chunks), CLIP_MODES[mode], float(threshold), _p(norm),
                                _stream(stream_of)), "gasfm_grad_clip")


def adam_control(ctl, sumsq, loss, lr, step, beta1, beta2, clip_mode, clip_th):
    """gasfm_adam_control: this step's gasfm_adam_ctl from device values (lr: a float or a 0-d fp32 device tensor)."""
    lr_dev = lr if torch.is_tensor(lr) else None
    check(lib().gasfm_adam_control(_p(ctl), _p(sumsq), _p(loss), _p(lr_dev), 0.0 if lr_dev is not None else float(lr),
                                   _p(step), float(beta1), float(beta2), CLIP_MODES[clip_mode], float(clip_th or 0.0),
                                   _stream(ctl)), "gasfm_adam_control")


def adam_step_ctl(tensors, chunks, n_chunks, ctl, beta1, beta2, eps, weight_decay, clip_mode, clip_th):
    """gasfm_adam_step_ctl: the Adam update with its step constants, skip flag and clip coefficient from ctl."""
    check(lib().gasfm_adam_step_ctl(_p(tensors), _p(chunks), int(n_chunks), _p(ctl), float(beta1), float(beta2),
                                    float(eps), float(weight_decay), CLIP_MODES[clip_mode], float(clip_th or 0.0),
                                    _stream(ctl)), "gasfm_adam_step_ctl")


def union_fill_pad(pd, out, stream_of):
    check(lib().gasfm_union_fill_pad(ctypes.byref(pd), ctypes.byref(out), _stream(stream_of)), "gasfm_union_fill_pad")


_SOS_TABLES_IN = ("cam_ptr", "pt_ptr", "soc32", "sop32", "cam32", "eoff")
_SOS_TABLES_I32 = ("ptrc", "ptrp", "ptre")
_SOS_TABLES_F64 = ("Es", "degc", "invc", "wc", "degp", "invp", "wp")
_SOS_TABLES_I64 = ("sop", "soe")


SosTables = _abi.structs["gasfm_sos_tables"]


def sos_tables_args(cam_ptr, pt_ptr, soc32, sop32, cam32, eoff, out):
    """The gasfm_sos_tables of a union's static buffers (int32: cam_ptr [M + 1], pt_ptr [N + 1],
    soc32 [M], sop32 [N], cam32 [E], eoff [S + 1]) and its table buffers ``out`` (attributes ptrc /
    ptrp / ptre int32 [S + 1]; Es [S], degc / invc / wc [M], degp / invp / wp [N] fp64; sop [N],
    soe [E] int64), every shape and type checked: built once per bucket, launched every step."""
    M, N, E, S = soc32.numel(), sop32.numel(), cam32.numel(), eoff.numel() - 1
    dev = soc32.device
    want = dict(cam_ptr=M + 1, pt_ptr=N + 1, soc32=M, sop32=N, cam32=E, eoff=S + 1, ptrc=S + 1, ptrp=S + 1,
                ptre=S + 1, Es=S, degc=M, invc=M, wc=M, degp=N, invp=N, wp=N, sop=N, soe=E)
    given = dict(cam_ptr=cam_ptr, pt_ptr=pt_ptr, soc32=soc32, sop32=sop32, cam32=cam32, eoff=eoff)
    if S < 1 or M < 1 or N < 1:
        raise ValueError(f"sos_union_tables: S={S} M={M} N={N}")
    t = SosTables()
    for group, dtype in ((_SOS_TABLES_IN, torch.int32), (_SOS_TABLES_I32, torch.int32),
                         (_SOS_TABLES_F64, torch.float64), (_SOS_TABLES_I64, torch.int64)):
        for k in group:
            v = given[k] if k in given else getattr(out, k)
            if not (v.is_cuda and v.device == dev and v.dtype == dtype and v.dim() == 1 and v.is_contiguous()
                    and v.numel() == want[k]):
                raise ValueError(f"sos_union_tables: {k} must be a contiguous {dtype} CUDA vector of {want[k]} entries")
            setattr(t, k, v.data_ptr())
    t.M, t.N, t.E, t.S = M, N, E, S
    return t


def sos_union_tables(t, stream_of):
    """One launch of gasfm_sos_union_tables on ``stream_of``'s current stream (t: sos_tables_args)."""
    check(lib().gasfm_sos_union_tables(ctypes.byref(t), _stream(stream_of)), "gasfm_sos_union_tables")


# ---------------------------------------------------------------- batched single-row problems (global hub)
def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def _ints(v):
    return (ctypes.c_int32 * len(v))(*v)


def gvec_multi_fwd(probs, eps):
    """probs: [(x, ln_w, ln_b, W, b, res, y)]; x / res / y 1-D rows, W [N, K]."""
    cols = list(zip(*probs))
    for W in cols[3]:
        _req(W, "W")
    K = [W.shape[1] for W in cols[3]]
    N = [W.shape[0] for W in cols[3]]
    st = lib().gasfm_gvec_multi_fwd(len(probs), *[_ptrs(c) for c in cols], _ints(K), _ints(N), eps,
                                    _stream(cols[0][0]))
    check(st, "gasfm_gvec_multi_fwd")


def gvec_multi_bwd(probs, groups, eps):
    """probs: [(dy, x, ln_w, ln_b, W, dW, db, dgam, dbet, part)]; groups: [(p0, np, dres, dx)]."""
    dy, x, lw, lb, W, dW, db, dg, dbt, part = (list(c) for c in zip(*probs))
    K = [w.shape[1] for w in W]
    N = [w.shape[0] for w in W]
    p0, npr, dres, dx = (list(c) for c in zip(*groups))
    st = lib().gasfm_gvec_multi_bwd(len(probs), _ptrs(dy), _ptrs(x), _ptrs(lw), _ptrs(lb), _ptrs(W), _ints(K),
                                    _ints(N), _ptrs(dW), _ptrs(db), _ptrs(dg), _ptrs(dbt), _ptrs(part), len(groups),
                                    _ints(p0), _ints(npr), _ptrs(dres), _ptrs(dx), eps, _stream(x[0]))
    check(st, "gasfm_gvec_multi_bwd")


# ---------------------------------------------------------------- the global node's chain (global_chain.hip)
_GC_W = ("W1", "b1", "gM", "bM", "W2", "b2", "gA", "bA", "WA", "gB", "bB", "WB", "bWB", "gC", "bC", "WC", "bWC",
         "WD", "bD", "WE", "bE")
_GC_D = tuple("d" + k for k in _GC_W)


_GC_SHADOW = ("W1", "W2", "WA", "WB", "WC", "WD", "WE")  # the weights with an optional bf16 shadow


_GChain = _abi.structs["gasfm_gchain"]
_GChainGrads = _abi.structs["gasfm_gchain_grads"]
GCHAIN_MAX_ROWS = _C["GASFM_GCHAIN_MAX_ROWS"]


def gchain_struct(w, eps_m, eps_h, shadows=None, rows=1):
    """gasfm_gchain of the weights dict w (keys _GC_W; the hub's B..E absent for the last block);
    shadows: dict weight key -> its bf16 shadow (BASELINE config 5) or None."""
    c = _GChain()
    W1, WA = w["W1"], w["WA"]
    hub = w.get("WB") is not None
    dims = dict(G=W1.shape[0], Kc=W1.shape[1], NA=WA.shape[0], NB=w["WB"].shape[0] if hub else 0,
                NC=w["WC"].shape[0] if hub else 0, ND=w["WD"].shape[0] if hub else 0,
                NE=w["WE"].shape[0] if hub else 0)
    for k, v in dims.items():
        setattr(c, k, int(v))
    c.eps_m, c.eps_h = float(eps_m), float(eps_h)
    for k in _GC_W:
        t = w.get(k)
        if t is not None:
            _req(t, k)
            setattr(c, k, t.data_ptr())
    for k, t in (shadows or {}).items():
        if t is not None:
            if t.dtype != torch.bfloat16 or not t.is_contiguous() or t.shape != w[k].shape:
                raise ValueError(f"gchain: the bf16 shadow of {k} must be a contiguous bf16 tensor of its shape")
            setattr(c, k + "h", t.data_ptr())
    if not 1 <= rows <= GCHAIN_MAX_ROWS:
        raise ValueError(f"gchain: {rows} rows (1..{GCHAIN_MAX_ROWS})")
    c.rows = int(rows)
    return c


def gchain_fwd(c, xcat, prev, x1, g, sg, xv, xp, xrv, xrp):
    st = lib().gasfm_gchain_fwd(ctypes.addressof(c), _p(xcat), _p(prev), _p(x1), _p(g), _p(sg), _p(xv), _p(xp),
                                _p(xrv), _p(xrp), _stream(g))
    check(st, "gasfm_gchain_fwd")


def gchain_bwd(c, xcat, x1, g, xv, xp, dskip, dsg, dxrv, dxrp, dxcat, dprev, grads):
    """grads: dict d<weight> -> tensor (gradient buffers to fill)."""
    d = _GChainGrads()
    for k in _GC_D:
        t = grads.get(k)
        if t is not None:
            setattr(d, k, t.data_ptr())
    L = lib()
    ws = torch.empty(int(L.gasfm_gchain_scratch_floats(ctypes.addressof(c))), dtype=torch.float32, device=g.device)
    cnt = _counters(g.device, L.gasfm_gchain_counters(ctypes.addressof(c)))
    st = L.gasfm_gchain_bwd(ctypes.addressof(c), _p(xcat), _p(x1), _p(g), _p(xv), _p(xp), _p(dskip), _p(dsg),
                            _p(dxrv), _p(dxrp), _p(dxcat), _p(dprev), ctypes.addressof(d), _p(ws), _p(cnt),
                            _stream(g))
    check(st, "gasfm_gchain_bwd")


# ---------------------------------------------------------------- global GATv2 convs (global_attn.hip)
_GattProb = _abi.structs["gasfm_gatt_prob"]


def _gatt_probs(probs):
    """probs: dicts with XL [rows, HC] (unit column stride), src (int32 CUDA vector or None), S, XR,
    att, bias and the outputs of the direction; returns a ctypes array."""
    arr = (_GattProb * len(probs))()
    for q, d in enumerate(probs):
        XL = d["XL"]
        if not XL.is_cuda or XL.dtype != torch.float32 or XL.stride(1) != 1:
            raise TypeError("gatt: XL must be a float32 CUDA tensor with unit column stride")
        src = d.get("src")
        if src is not None and (src.dtype != torch.int32 or not src.is_contiguous()):
            raise TypeError("gatt: src must be a contiguous int32 tensor")
        a = arr[q]
        a.XL, a.ldXL, a.src, a.S, a.HC = XL.data_ptr(), XL.stride(0), _p(src), int(d["S"]), int(d["att"].numel())
        for k in ("XR", "att", "bias", "out", "smax", "ssum", "part", "gout", "dXR", "datt"):
            setattr(a, k, _p(d.get(k)))
        dXL = d.get("dXL")
        if dXL is not None:
            if dXL.stride(1) != 1:
                raise TypeError("gatt: dXL must have unit column stride")
            a.dXL, a.ldDXL = dXL.data_ptr(), dXL.stride(0)
    return arr


def gatt_fwd(probs, slope):
    """One launch: both global convs' forward (gasfm_gatt_fwd)."""
    arr = _gatt_probs(probs)
    L = lib()
    dev = probs[0]["XL"].device
    ws = torch.empty(int(L.gasfm_gatt_scratch_floats(len(probs), ctypes.addressof(arr))), dtype=torch.float32, device=dev)
    cnt = _counters(dev, int(L.gasfm_gatt_counters(len(probs), ctypes.addressof(arr))))
    check(L.gasfm_gatt_fwd(len(probs), ctypes.addressof(arr), float(slope), _p(ws), _p(cnt), _stream(probs[0]["XL"])),
          "gasfm_gatt_fwd")


def gatt_bwd(probs, slope):
    """One launch: both global convs' backward (gasfm_gatt_bwd)."""
    arr = _gatt_probs(probs)
    L = lib()
    dev = probs[0]["XL"].device
    ws = torch.empty(int(L.gasfm_gatt_scratch_floats(len(probs), ctypes.addressof(arr))), dtype=torch.float32, device=dev)
    cnt = _counters(dev, int(L.gasfm_gatt_counters(len(probs), ctypes.addressof(arr))))
    check(L.gasfm_gatt_bwd(len(probs), ctypes.addressof(arr), float(slope), _p(ws), _p(cnt), _stream(probs[0]["XL"])),
          "gasfm_gatt_bwd")


def gatt_merge(probs, nrows, stride, unpack=None):
    """One launch: merge the nrows gathered partial rows of each problem (probs[q]["part"]: the first
    row; rank r's at + r * stride floats) into its out / smax / ssum (gasfm_gatt_merge).  unpack =
    (G, blk, roff, chunk, dst [m, width]): the same launch also copies every rank's own rows out of
    the gathered send blocks G (gasfm_gatt_merge_unpack)."""
    arr = (_GattProb * len(probs))()
    for q, d in enumerate(probs):
        a = arr[q]
        a.HC = int(d["bias"].numel())
        for k in ("bias", "out", "smax", "ssum", "part"):
            setattr(a, k, _p(d[k]))
    if unpack is None:
        check(lib().gasfm_gatt_merge(len(probs), ctypes.addressof(arr), int(nrows), int(stride), _stream(d["bias"])),
              "gasfm_gatt_merge")
        return
    G, blk, roff, chunk, dst = unpack
    _exchange_args(G, dst, None)
    check(lib().gasfm_gatt_merge_unpack(len(probs), ctypes.addressof(arr), int(nrows), int(stride), _p(G), int(nrows),
                                        int(blk), int(roff), int(chunk), int(dst.shape[1]), int(dst.shape[0]), _p(dst),
                                        dst.stride(0) if dst.shape[0] > 1 else dst.shape[1], _stream(G)),
          "gasfm_gatt_merge_unpack")


def _exchange_args(G, rows_dst, sum_dst):
    for t, nm in ((G, "G"), (rows_dst, "rows_dst"), (sum_dst, "sum_dst")):
        if t is not None and (not t.is_cuda or t.dtype != torch.float32 or t.stride(-1) != 1):
            raise TypeError(f"exchange_unpack: {nm} must be float32 CUDA with unit column stride")


def exchange_unpack(G, W, blk, rows=None, sums=None):
    """Unpack W gathered send blocks of blk floats (gasfm_exchange_unpack): rows = (roff, chunk, dst
    [m, width]) copies every rank's own rows into dst, sums = (soff, dst [sn]) the rank-order sum of
    the W partial vectors."""
    roff, chunk, rdst = rows if rows is not None else (0, 1, None)
    soff, sdst = sums if sums is not None else (0, None)
    _exchange_args(G, rdst, sdst)
    width = int(rdst.shape[1]) if rdst is not None else 4
    m = int(rdst.shape[0]) if rdst is not None else 0
    ld = (rdst.stride(0) if m > 1 else width) if rdst is not None else 4
    check(lib().gasfm_exchange_unpack(_p(G), int(W), int(blk), int(roff), int(chunk), width, m, _p(rdst), ld,
                                      int(soff), int(sdst.numel()) if sdst is not None else 0, _p(sdst), _stream(G)),
          "gasfm_exchange_unpack")


# ---------------------------------------------------------------- device scene builder (scene_build.hip)
def scan_i32(x):
    """Exclusive scan of an int32 CUDA vector: returns out[L + 1] (out[L] = total)."""
    _i32vec(x, "scan input")
    out = torch.empty(x.shape[0] + 1, dtype=torch.int32, device=x.device)
    check(lib().gasfm_scan_i32(_p(x), x.shape[0], _p(out), _stream(x)), "gasfm_scan_i32")
    return out


# ---------------------------------------------------------------- outlier injection (outliers.hip)
def _dev_check(what, *ts):
    for name, t, dt in ts:
        if t is not None and (not t.is_cuda or t.dtype != dt or not t.is_contiguous()):
            raise TypeError(f"{what}: {name} must be a contiguous {dt} CUDA tensor")


def outlier_counts(state, cam_ptr, pt_ptr, perm, m, n):
    """Inliers per view / per point and their minima: (cam_in [m], pt_in [n], mins [2]) int32."""
    _dev_check("outlier_counts", ("state", state, torch.uint8), ("cam_ptr", cam_ptr, torch.int32),
               ("pt_ptr", pt_ptr, torch.int32), ("perm", perm, torch.int32))
    if cam_ptr.shape[0] != m + 1 or pt_ptr.shape[0] != n + 1:
        raise ValueError("outlier_counts: cam_ptr / pt_ptr must have m + 1 / n + 1 entries")
    dev = state.device
    cam_in = torch.empty(m, dtype=torch.int32, device=dev)
    pt_in = torch.empty(n, dtype=torch.int32, device=dev)
    mins = torch.empty(2, dtype=torch.int32, device=dev)
    check(lib().gasfm_outlier_counts(_p(state), _p(cam_ptr), _p(pt_ptr), _p(perm), m, n, _p(cam_in), _p(pt_in),
                                     _p(mins), _stream(state)), "gasfm_outlier_counts")
    return cam_in, pt_in, mins


def outlier_mark(state, cam, pt, cam_in, pt_in, mode, counts=None):
    """init (mode 0) / blacklist (mode 1) pass over the edge classes; returns counts [4] int32."""
    _dev_check("outlier_mark", ("state", state, torch.uint8), ("cam", cam, torch.int64), ("pt", pt, torch.int64),
               ("cam_in", cam_in, torch.int32), ("pt_in", pt_in, torch.int32))
    E = state.shape[0]
    if cam.shape[0] != E or pt.shape[0] != E:
        raise ValueError("outlier_mark: cam / pt must have one entry per edge")
    if counts is None:
        counts = torch.empty(4, dtype=torch.int32, device=state.device)
    check(lib().gasfm_outlier_mark(_p(state), _p(cam), _p(pt), _p(cam_in), _p(pt_in), E, mode, _p(counts),
                                   _stream(state)), "gasfm_outlier_mark")
    return counts


def outlier_moments(values, state, cam_ptr, m):
    """(mu [m, 2], sigma [m, 2, 2], scale_tril [m, 2, 2], pivots [m, 2] int32) of the inliers."""
    _dev_check("outlier_moments", ("values", values, torch.float32), ("state", state, torch.uint8),
               ("cam_ptr", cam_ptr, torch.int32))
    if values.dim() != 2 or values.shape[1] != 2 or values.shape[0] != state.shape[0] or cam_ptr.shape[0] != m + 1:
        raise ValueError("outlier_moments: values [E, 2], state [E], cam_ptr [m + 1]")
    dev = values.device
    mu = torch.empty((m, 2), dtype=torch.float32, device=dev)
    sigma = torch.empty((m, 2, 2), dtype=torch.float32, device=dev)
    tril = torch.empty((m, 2, 2), dtype=torch.float32, device=dev)
    piv = torch.empty((m, 2), dtype=torch.int32, device=dev)
    check(lib().gasfm_outlier_moments(_p(values), _p(state), _p(cam_ptr), m, _p(mu), _p(sigma), _p(tril), _p(piv),
                                      _stream(values)), "gasfm_outlier_moments")
    return mu, sigma, tril, piv


def outlier_apply(idx, cam, pt, z, mu, tril, M, pix=None):
    """Write mu[cam] + scale_tril[cam] z[k] for the outlier edges idx (ascending) into M (and pix)."""
    _dev_check("outlier_apply", ("idx", idx, torch.int64), ("cam", cam, torch.int64), ("pt", pt, torch.int64),
               ("z", z, torch.float32), ("mu", mu, torch.float32), ("scale_tril", tril, torch.float32),
               ("pix", pix, torch.float32))
    _check_M(M, "outlier_apply")
    k = idx.shape[0]
    if z.numel() != 2 * k:
        raise ValueError(f"outlier_apply: z has {z.numel()} values for {k} outliers")
    m = M.shape[0] // 2
    if mu.shape != (m, 2) or tril.shape != (m, 2, 2):
        raise ValueError("outlier_apply: mu [m, 2], scale_tril [m, 2, 2]")
    check(lib().gasfm_outlier_apply(_p(idx), k, _p(cam), _p(pt), _p(z), _p(mu), _p(tril), _p(M), M.stride(0),
                                    _p(pix), _stream(M)), "gasfm_outlier_apply")


def _check_M(M, what):
    if not M.is_cuda or M.dtype != torch.float32 or M.dim() != 2 or M.stride(1) != 1 or M.shape[0] % 2:
        raise TypeError(f"{what}: M must be a float32 CUDA [2m, n] matrix with unit column stride "
                        "(no CPU fallback)")


def scene_mask(M):
    """gasfm_scene_mask on a dense M: (mask [m*W] int64 bits, pt_valid [W], pt_count int32 [n] (views of
    points with >= 2, else 0), tile_base int32 [tiles + 1])."""
    _check_M(M, "scene_mask")
    m, n = M.shape[0] // 2, M.shape[1]
    L = lib()
    dev = M.device
    W, T = L.gasfm_scene_mask_words(n), L.gasfm_scene_tiles(m, n)
    i32 = dict(dtype=torch.int32, device=dev)
    mask = torch.empty(m * W, dtype=torch.int64, device=dev)
    pt_valid = torch.empty(W, dtype=torch.int64, device=dev)
    view_count, pt_count = torch.empty(n, **i32), torch.empty(n, **i32)
    tile_count, tile_base = torch.empty(T, **i32), torch.empty(T + 1, **i32)
    check(L.gasfm_scene_mask(_p(M), M.stride(0), m, n, _p(mask), _p(view_count), _p(pt_valid), _p(pt_count),
                             _p(tile_count), _p(tile_base), _stream(M)), "gasfm_scene_mask")
    return mask, pt_valid, pt_count, tile_base


def scene_homography(M, Ns, R, Ninv):
    """Rotational homography augmentation of a dense M (gasfm_scene_homography): new [2m, n] M."""
    _check_M(M, "scene_homography")
    m, n = M.shape[0] // 2, M.shape[1]
    for t, name in ((Ns, "Ns"), (R, "R"), (Ninv, "Ninv")):
        if not t.is_cuda or t.dtype != torch.float32 or tuple(t.shape) != (m, 3, 3) or not t.is_contiguous():
            raise TypeError(f"scene_homography: {name} must be a contiguous float32 CUDA [m, 3, 3] tensor")
    mask, pt_valid, _, _ = scene_mask(M)
    out = torch.empty_like(M)
    check(lib().gasfm_scene_homography(_p(M), M.stride(0), m, n, _p(mask), _p(pt_valid), _p(Ns), _p(R), _p(Ninv),
                                       _p(out), out.stride(0), _stream(M)), "gasfm_scene_homography")
    return out


def scene_build(M, Ns=None):
    """Dense M [2m, n] (CUDA fp32) -> dict of device tensors: cam, pt (int64 [E]), values [E, 2],
    pt_count (int32 [n], the reference's cam_per_pts), cam_ptr (int32 [m+1]), pt_ptr (int32 [n+1]),
    perm / pos (int32 [E]).  One host sync (E sizes the edge buffers)."""
    _check_M(M, "scene_build")
    m, n = M.shape[0] // 2, M.shape[1]
    if Ns is not None:
        if not Ns.is_cuda or Ns.dtype != torch.float32 or tuple(Ns.shape) != (m, 3, 3):
            raise TypeError("scene_build: Ns must be a float32 CUDA [m, 3, 3] tensor")
        Ns = Ns.contiguous()
    L = lib()
    dev = M.device
    T = L.gasfm_scene_tiles(m, n)
    i32 = dict(dtype=torch.int32, device=dev)
    mask, pt_valid, pt_count, tile_base = scene_mask(M)
    st = _stream(M)
    W = L.gasfm_scene_mask_words(n)
    E = int(tile_base[T].item())
    cam = torch.empty(E, dtype=torch.int64, device=dev)
    pt = torch.empty(E, dtype=torch.int64, device=dev)
    vals = torch.empty((E, 2), dtype=torch.float32, device=dev)
    word_base = torch.empty(m * W, **i32)
    check(L.gasfm_scene_emit(_p(M), M.stride(0), _p(Ns) if Ns is not None else None, m, n, _p(mask), _p(pt_valid),
                             _p(tile_base), _p(cam), _p(pt), _p(vals), _p(word_base), st), "gasfm_scene_emit")
    pt_ptr = scan_i32(pt_count)
    perm, pos = torch.empty(E, **i32), torch.empty(E, **i32)
    if E:
        check(L.gasfm_scene_point_csr(_p(mask), _p(pt_valid), _p(word_base), _p(pt_ptr), m, n, _p(perm), _p(pos),
                                      st), "gasfm_scene_point_csr")
    cam_ptr = tile_base[0::T // m].contiguous() if T else torch.zeros(m + 1, **i32)
    return {"cam": cam, "pt": pt, "values": vals, "pt_count": pt_count, "cam_ptr": cam_ptr, "pt_ptr": pt_ptr,
            "perm": perm, "pos": pos}


# ---------------------------------------------------------------- point shard of a device scene (scene_shard.hip)
def _edge_ids(t, name, what):
    """(tensor, is64) of a per-edge int32 / int64 CUDA index vector."""
    if not t.is_cuda or t.dtype not in (torch.int32, torch.int64) or t.dim() != 1 or not t.is_contiguous():
        raise TypeError(f"{what}: {name} must be a contiguous int32 or int64 CUDA vector")
    return t, int(t.dtype == torch.int64)


def scene_shard_bounds(pt_ptr, world):
    """distributed.partition_points over the point CSR: int32 [world + 1] device boundaries."""
    _dev_check("scene_shard_bounds", ("pt_ptr", pt_ptr, torch.int32))
    if world < 1 or pt_ptr.dim() != 1 or pt_ptr.shape[0] < 1:
        raise ValueError("scene_shard_bounds: world >= 1 and pt_ptr [n + 1]")
    bounds = torch.empty(world + 1, dtype=torch.int32, device=pt_ptr.device)
    check(lib().gasfm_scene_shard_bounds(_p(pt_ptr), pt_ptr.shape[0] - 1, world, _p(bounds), _stream(pt_ptr)),
          "gasfm_scene_shard_bounds")
    return bounds


def scene_shard_ranges(cam_ptr, pt_ptr, pt, bounds, rank, c0=0, c1=0):
    """The per-camera runs of rank ``rank``'s points (bounds: int32 device boundaries) and the scalars
    the host sizes the shard by: dict lo, count (int32 [m]), lcam_ptr (int32 [m + 1]), pts_per_cam
    (int64 [m]), valid_view (bool [m]), stats (int64 [9], gasfm_scene_shard_stats)."""
    what = "scene_shard_ranges"
    _dev_check(what, ("cam_ptr", cam_ptr, torch.int32), ("pt_ptr", pt_ptr, torch.int32), ("bounds", bounds, torch.int32))
    pt, is64 = _edge_ids(pt, "pt", what)
    m, n = cam_ptr.shape[0] - 1, pt_ptr.shape[0] - 1
    if m < 0 or n < 0 or not 0 <= rank < bounds.shape[0] - 1 or not 0 <= c0 <= c1 <= m:
        raise ValueError(f"{what}: rank {rank} of {bounds.shape[0] - 1}, cameras [{c0}, {c1}) of {m}")
    dev = cam_ptr.device
    L, st = lib(), _stream(cam_ptr)
    lo = torch.empty(m, dtype=torch.int32, device=dev)
    count = torch.empty(m, dtype=torch.int32, device=dev)
    ppc = torch.empty(m, dtype=torch.int64, device=dev)
    vv = torch.empty(m, dtype=torch.uint8, device=dev)
    stats = torch.empty(9, dtype=torch.int64, device=dev)
    check(L.gasfm_scene_shard_cam_range(_p(cam_ptr), _p(pt), is64, m, _p(bounds), rank, _p(lo), _p(count), _p(ppc),
                                        _p(vv), st), "gasfm_scene_shard_cam_range")
    check(L.gasfm_scene_shard_stats(_p(cam_ptr), m, _p(pt_ptr), n, _p(bounds), rank, c0, c1, _p(stats), st),
          "gasfm_scene_shard_stats")
    return {"lo": lo, "count": count, "lcam_ptr": scan_i32(count), "pts_per_cam": ppc, "valid_view": vv.view(torch.bool),
            "stats": stats}


def scene_shard_emit(r, pt, p0, E_loc, sources):
    """The local edges of scene_shard_ranges' result r: (sel int64 [E_loc], indices int64 [2, E_loc],
    cam32, pt32 int32 [E_loc], [the gathered rows of each [E, 2] fp32 array in ``sources`` (<= 3)])."""
    what = "scene_shard_emit"
    pt, is64 = _edge_ids(pt, "pt", what)
    if len(sources) > 3:
        raise ValueError(f"{what}: at most three source arrays")
    for s in sources:
        if not s.is_cuda or s.dtype != torch.float32 or s.dim() != 2 or s.shape != (pt.shape[0], 2) \
                or not s.is_contiguous():
            raise TypeError(f"{what}: sources must be contiguous float32 CUDA [E, 2] arrays")
    dev = pt.device
    m = r["lo"].shape[0]
    sel = torch.empty(E_loc, dtype=torch.int64, device=dev)
    indices = torch.empty((2, E_loc), dtype=torch.int64, device=dev)
    cam32 = torch.empty(E_loc, dtype=torch.int32, device=dev)
    pt32 = torch.empty(E_loc, dtype=torch.int32, device=dev)
    dst = [torch.empty((E_loc, 2), dtype=torch.float32, device=dev) for _ in sources]
    sp = [_p(s) for s in sources] + [None] * (3 - len(sources))
    dp = [_p(d) for d in dst] + [None] * (3 - len(dst))
    check(lib().gasfm_scene_shard_emit(_p(r["lcam_ptr"]), _p(r["lo"]), m, _p(pt), is64, E_loc, p0, sp[0], sp[1], sp[2],
                                       _p(sel), _p(indices), _p(cam32), _p(pt32), dp[0], dp[1], dp[2], _stream(pt)),
          "gasfm_scene_shard_emit")
    return sel, indices, cam32, pt32, dst


def scene_shard_point_csr(r, pt_ptr, perm, cam, p0, p1, E_loc):
    """The local point CSR of scene_shard_ranges' result r: (lpt_ptr int32 [n_loc + 1], cam_per_pts
    int64 [n_loc], valid_pt bool [n_loc], perm, pos int32 [E_loc]).  perm: the global CSR's, or None."""
    what = "scene_shard_point_csr"
    _dev_check(what, ("pt_ptr", pt_ptr, torch.int32), ("perm", perm, torch.int32))
    cam, is64 = _edge_ids(cam, "cam", what)
    n_loc = p1 - p0
    if not 0 <= p0 <= p1 < pt_ptr.shape[0] or (perm is not None and perm.shape[0] != cam.shape[0]):
        raise ValueError(f"{what}: points [{p0}, {p1}) of {pt_ptr.shape[0] - 1}; perm must have one entry per edge")
    dev = cam.device
    i32 = dict(dtype=torch.int32, device=dev)
    lpt_ptr = torch.empty(n_loc + 1, **i32)
    cpp = torch.empty(n_loc, dtype=torch.int64, device=dev)
    vp = torch.empty(n_loc, dtype=torch.uint8, device=dev)
    lperm, lpos = torch.empty(E_loc, **i32), torch.empty(E_loc, **i32)
    check(lib().gasfm_scene_shard_point_csr(_p(pt_ptr), _p(perm), _p(cam), is64, _p(r["lcam_ptr"]), _p(r["lo"]), p0,
                                            n_loc, E_loc, _p(lpt_ptr), _p(cpp), _p(vp), _p(lperm), _p(lpos),
                                            _stream(cam)), "gasfm_scene_shard_point_csr")
    return lpt_ptr, cpp, vp.view(torch.bool), lperm, lpos


# ---------------------------------------------------------------- per-edge depth targets (depth_targets.hip)
def _depth_edges(what, cam, pt):
    cam, is64 = _edge_ids(cam, "cam", what)
    pt, pis64 = _edge_ids(pt, "pt", what)
    if is64 != pis64 or cam.shape != pt.shape:
        raise TypeError(f"{what}: cam and pt must have one dtype and one length")
    return cam, pt, is64


def _depth_part(E, dev):
    """(per-wave count scratch, the [1] int32 count) of a depth_targets.hip kernel over E edges."""
    part = torch.empty(int(lib().gasfm_depth_part_slots(E)), dtype=torch.int32, device=dev)
    return part, torch.zeros(1, dtype=torch.int32, device=dev)


def depth_targets(a, X, cam, pt, out=None):
    """d[e] = a[cam[e]] . X[pt[e]] (gasfm_depth_targets): (d [E] float32, bad [1] int32 = the number of
    edges whose depth is not finite or not > 0, on the device).  a [m, 4], X [n, 4] float32."""
    what = "depth_targets"
    cam, pt, is64 = _depth_edges(what, cam, pt)
    for t, name in ((a, "a"), (X, "X")):
        if not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 4 or not t.is_contiguous():
            raise TypeError(f"{what}: {name} must be a contiguous float32 CUDA [rows, 4] tensor")
    E = cam.shape[0]
    d = torch.empty(E, dtype=torch.float32, device=cam.device) if out is None else out
    _dev_check(what, ("out", d, torch.float32))
    if d.shape != (E,):
        raise ValueError(f"{what}: out must have one entry per edge")
    part, bad = _depth_part(E, cam.device)
    check(lib().gasfm_depth_targets(_p(a), a.shape[0], _p(X), X.shape[0], _p(cam), _p(pt), is64, E, _p(d), _p(part),
                                    _p(bad), _stream(cam)), "gasfm_depth_targets")
    return d, bad


def depth_gather(pcam_ptr, ppt, pd, view_idx, keep, cam, pt, out=None):
    """The sampled scene's per-edge depths from its parent's (gasfm_depth_gather): (d [E] float32,
    missing [1] int32 = the number of sampled edges without a parent edge, on the device)."""
    what = "depth_gather"
    cam, pt, is64 = _depth_edges(what, cam, pt)
    ppt, pis64 = _edge_ids(ppt, "parent pt", what)
    _dev_check(what, ("parent cam_ptr", pcam_ptr, torch.int32), ("parent depths", pd, torch.float32),
               ("view_idx", view_idx, torch.int64), ("keep", keep, torch.int64))
    if pcam_ptr.dim() != 1 or pcam_ptr.shape[0] < 1 or pd.shape != ppt.shape or view_idx.dim() != 1 or keep.dim() != 1:
        raise ValueError(f"{what}: parent cam_ptr [m + 1], parent pt / depths [E], view_idx [m'], keep [n']")
    E = cam.shape[0]
    d = torch.empty(E, dtype=torch.float32, device=cam.device) if out is None else out
    _dev_check(what, ("out", d, torch.float32))
    if d.shape != (E,):
        raise ValueError(f"{what}: out must have one entry per edge")
    part, missing = _depth_part(E, cam.device)
    check(lib().gasfm_depth_gather(_p(pcam_ptr), _p(ppt), pis64, _p(pd), pcam_ptr.shape[0] - 1, ppt.shape[0],
                                   _p(view_idx), _p(keep), view_idx.shape[0], keep.shape[0], _p(cam), _p(pt), is64, E,
                                   _p(d), _p(part), _p(missing), _stream(cam)), "gasfm_depth_gather")
    return d, missing


def depth_rescale(d, cam, pt, M, Ns, R, out=None):
    """d[e] / z_old * z_new of the rotational homography augmentation (gasfm_depth_rescale), the old
    pixel measurements read from the un-augmented dense M [2m, n]."""
    what = "depth_rescale"
    _check_M(M, what)
    cam, pt, is64 = _depth_edges(what, cam, pt)
    m, n = M.shape[0] // 2, M.shape[1]
    for t, name in ((Ns, "Ns"), (R, "R")):
        if not t.is_cuda or t.dtype != torch.float32 or tuple(t.shape) != (m, 3, 3) or not t.is_contiguous():
            raise TypeError(f"{what}: {name} must be a contiguous float32 CUDA [m, 3, 3] tensor")
    _dev_check(what, ("d", d, torch.float32))
    E = cam.shape[0]
    res = torch.empty(E, dtype=torch.float32, device=cam.device) if out is None else out
    _dev_check(what, ("out", res, torch.float32))
    if d.shape != (E,) or res.shape != (E,):
        raise ValueError(f"{what}: d and out must have one entry per edge")
    check(lib().gasfm_depth_rescale(_p(d), _p(cam), _p(pt), is64, E, _p(M), M.stride(0), m, n, _p(Ns), _p(R), _p(res),
                                    _stream(cam)), "gasfm_depth_rescale")
    return res


def sum_n(tensors):
    """Elementwise sum of same-shape contiguous fp32 CUDA tensors in one pass (gasfm_sum_n)."""
    t0 = tensors[0]
    for t in tensors:
        _req(t, "sum_n input")
        if t.shape != t0.shape:
            raise ValueError("sum_n: shapes differ")
    if t0.numel() % 4:  # the kernel streams float4s (odd E): pairwise adds on the device
        out = tensors[0].clone()
        for t in tensors[1:]:
            out += t
        return out
    out = torch.empty_like(t0)
    st = lib().gasfm_sum_n(len(tensors), _ptrs(tensors), t0.numel(), _p(out), _stream(t0))
    check(st, "gasfm_sum_n")
    return out


def _gemm(fn, what, a, b, cin=None, bias=None, out=None):
    for t, nm in ((a, what + " a"), (b, what + " b")):
        if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 2):
            raise ValueError(f"{nm}: fp32 CUDA matrix required")
    M, K = a.shape
    K2, N = b.shape
    if K2 != K:
        raise ValueError(f"{what}: inner dimensions {K} and {K2} differ")
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    if cin is not None and (cin.shape != (M, N) or cin.stride(1) != 1):
        raise ValueError(f"{what}: cin must be [M, N] with unit column stride")
    if bias is not None and (bias.shape != (N,) or not bias.is_contiguous()):
        raise ValueError(f"{what}: bias must be a contiguous [N] vector")
    if out.shape != (M, N) or out.stride(1) != 1:
        raise ValueError(f"{what}: out must be [M, N] with unit column stride")
    st = fn(M, N, K, _p(a), a.stride(0), a.stride(1), _p(b), b.stride(0), b.stride(1), _p(cin),
            cin.stride(0) if cin is not None else 0, _p(bias), _p(out), out.stride(0), _stream(out))
    check(st, what)
    return out


def gemm_bf16(a, b, cin=None, bias=None, out=None):
    """out = a @ b (+ cin) (+ bias) on bf16 MFMA with fp32 accumulation (gasfm_gemm_bf16).

    a [M, K], b [K, N]: fp32 CUDA tensors, each with a unit stride along one dimension (plain
    row-major tensors and their .t() views both qualify: x @ W.t(), dy @ W, dy.t() @ x)."""
    return _gemm(lib().gasfm_gemm_bf16, "gasfm_gemm_bf16", a, b, cin, bias, out)


def gemm_f32_smallm(a, b, cin=None, bias=None, out=None):
    """out = a @ b (+ cin) (+ bias) on the small-row-count fp32 MFMA kernels (csrc/gemm_smallm.hip),
    or None when the operand form / shape is not one of theirs: a @ W.t() (mode 0: a, W row-major),
    a @ W (mode 1, no epilogue), A.t() @ B (mode 2: A, B row-major, short K, no epilogue)."""
    if not (a.is_cuda and b.is_cuda and a.dtype == torch.float32 and b.dtype == torch.float32
            and a.dim() == 2 and b.dim() == 2 and a.shape[1] == b.shape[0]):
        return None
    M, K = a.shape
    N = b.shape[1]
    L = lib()
    if a.stride(1) == 1 and a.stride(0) % 4 == 0:
        if b.stride(0) == 1 and b.stride(1) % 4 == 0:  # b = W.t(), W [N, K] row-major
            mode, A, lda, B, ldb = 0, a, a.stride(0), b, b.stride(1)
        elif b.stride(1) == 1 and cin is None and bias is None:  # b = W [K, N] row-major
            mode, A, lda, B, ldb = 1, a, a.stride(0), b, b.stride(0)
        else:
            return None
        I, J = M, N
    elif a.stride(0) == 1 and b.stride(1) == 1 and cin is None and bias is None:  # a = A.t(), A [K, M]
        mode, A, lda, B, ldb = 2, a, a.stride(1), b, b.stride(0)
        I, J = M, N
    else:
        return None
    # modes 0 / 1 read float4 runs of A (and of W in mode 0): a misaligned view falls back to hipBLASLt
    if mode in (0, 1) and (A.data_ptr() % 16 or (mode == 0 and B.data_ptr() % 16)):
        return None
    if not L.gasfm_gemm_f32_smallm_ok(mode, I, J, K):
        return None
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    if out.shape != (M, N) or out.stride(1) != 1 or (cin is not None and (cin.shape != (M, N) or cin.stride(1) != 1)):
        return None
    if bias is not None and (bias.shape != (N,) or not bias.is_contiguous()):
        return None
    st = L.gasfm_gemm_f32_smallm(mode, I, J, K, _p(A), lda, _p(B), ldb, _p(bias), _p(cin),
                                 cin.stride(0) if cin is not None else 0, _p(out), out.stride(0), _stream(out))
    check(st, "gasfm_gemm_f32_smallm")
    return out


def gemm_f32(a, b, cin=None, bias=None, out=None):
    """out = a @ b (+ cin) (+ bias) in fp32 on v_mfma_f32_16x16x4_f32 (gasfm_gemm_f32); same
    operand rules as gemm_bf16.  out may be cin (accumulate in place)."""
    return _gemm(lib().gasfm_gemm_f32, "gasfm_gemm_f32", a, b, cin, bias, out)

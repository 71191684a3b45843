"""The small-m view chain (csrc/view_chain.hip: m <= 256 camera rows, D in {256, 512, 1024}) at every
width, at the edges of its 16-row tiles and of its KQ classes, with guarded output buffers and with a
poisoned workspace; and csrc/view_block.hip at the first row count past the chain.

Reference and bars are those of test_gpu_view_block.py (the fp64 torch composition of the
reference's ops; outputs 2e-5 * max|ref| + 1e-5, gradients normwise 1e-4 * |ref| + 1e-6).

Instantiations reached.  KU = D / 128 sets the loads per thread and the LDS staging of every chain
kernel (vc_tail_fwd<KU, prev>, vc_hub_fwd<KU>, vc_hub_bwd2<KU>) and ngrp = D / 128 of vc_tail_bwd2;
KQ = ceil-class of the row count (m <= 64: 4, m <= 128: 8, else 16) is the K depth of the
weight-gradient role of vc_hub_bwd1<KU, KQ> and vc_tail_bwd1<KU, KQ>.  Every tail case launches
vc_tail_bwd1, every hub case vc_hub_bwd1, so both run all nine pairs:

    D     KU   m in                       KQ
    256   2    16, 64                     4
    256   2    65, 128                    8
    256   2    129, 255                   16
    512   4    1, 15, 16, 17, 64          4
    512   4    65, 128                    8
    512   4    129, 255, 256              16
    1024  8    16, 64                     4
    1024  8    65, 128                    8
    1024  8    129, 255                   16

The kernel-level shapes are (17, 512) -> (4, 4), (129, 256) -> (2, 16), (255, 1024) -> (8, 16): all
ragged, three KU values, T = 2, 9 and 16 row tiles.  m = 257 at D in {128, 512, 960} is the first row
count past the chain and runs the view_block.hip kernels + GEMMs.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from gasfm_amd import _native, view_block
from test_gpu_view_block import EPS, _check, hub_case, run_hub, run_tail, tail_case

pytestmark = pytest.mark.gpu

TR = 16
SENT = -12345.0
ROWS_512 = [1, 15, 16, 17, 64, 65, 128, 129, 255, 256]
ROWS_EDGE = [16, 64, 65, 128, 129, 255]
CHAIN_SHAPES = [(m, 512) for m in ROWS_512] + [(m, D) for D in (256, 1024) for m in ROWS_EDGE]
PAST_CHAIN = [(257, D) for D in (128, 512, 960)]
# one ragged and one tile-exact row count per width
TWICE = [(255, 256), (128, 256), (17, 512), (256, 512), (129, 1024), (64, 1024)]
KERNEL_SHAPES = [(17, 512), (129, 256), (255, 1024)]

# the fp64 compositions, shared by the tests of one shape (read only)
_tail_case = functools.lru_cache(maxsize=4)(tail_case)
_hub_case = functools.lru_cache(maxsize=4)(hub_case)


def _ids(shapes):
    return [f"m{m}-D{D}" for m, D in shapes]


# ------------------------------------------------------------------------------ autograd level
@pytest.mark.parametrize("shape", CHAIN_SHAPES + PAST_CHAIN, ids=_ids(CHAIN_SHAPES + PAST_CHAIN))
@pytest.mark.parametrize("with_prev", [True, False])
def test_tail_matches_fp64(device, shape, with_prev):
    y, _ = run_tail(device, _tail_case(*shape, with_prev))
    assert y.grad_fn._forward_cls is view_block.ViewTailFn
    assert y.grad_fn.chain == (shape in CHAIN_SHAPES)


@pytest.mark.parametrize("packed", [False, True])  # varies fastest: the two share one fp64 case
@pytest.mark.parametrize("with_skip", [True, False])
@pytest.mark.parametrize("shape", CHAIN_SHAPES + PAST_CHAIN, ids=_ids(CHAIN_SHAPES + PAST_CHAIN))
def test_hub_matches_fp64(device, shape, with_skip, packed):
    outs, _ = run_hub(device, _hub_case(*shape, with_skip), packed)
    assert outs[1].grad_fn._forward_cls is view_block.ViewHubFn
    assert outs[1].grad_fn.chain == (shape in CHAIN_SHAPES)


def _same_bits(names, a, b):
    bad = [n for n, p, q in zip(names, a, b) if not torch.equal(p, q)]
    assert not bad, f"not bitwise equal between two runs: {bad}"


@pytest.mark.parametrize("shape", TWICE, ids=_ids(TWICE))
def test_tail_two_runs_are_bitwise_equal(device, shape):
    case = _tail_case(*shape, True)
    runs = []
    for _ in range(2):
        y, got = run_tail(device, case)
        assert y.grad_fn.chain is True
        runs.append([y.detach()] + [t.grad for t in got])
    _same_bits(("view", "d prev", "d agg", "dWp", "dbp", "dgamma", "dbeta", "dWm", "dbm"), *runs)


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("shape", TWICE, ids=_ids(TWICE))
def test_hub_two_runs_are_bitwise_equal(device, shape, packed):
    case = _hub_case(*shape, True)
    runs = []
    for _ in range(2):
        outs, got = run_hub(device, case, packed)
        assert outs[1].grad_fn.chain is True
        runs.append([o.detach() for o in outs] + [t.grad for t in got])
    _same_bits(("skip", "SV", "XL", "XR", "dv", "dgC", "dbC", "dWv", "dWl", "dbl", "dgA", "dbA", "dWa", "dba", "dWr",
                "dbr"), *runs)


# -------------------------------------------------------------------------------- kernel level
def _guarded(rows, cols, device, extra=TR):
    """A contiguous [rows + extra, cols] buffer of the sentinel; (the buffer, its [:rows] view)."""
    full = torch.full((rows + extra, cols), SENT, dtype=torch.float32, device=device)
    return full, full[:rows]


def _nan(D, device):
    return torch.full((D, D), float("nan"), dtype=torch.float32, device=device)


def _check_guards(bufs, what):
    """bufs: name -> (full buffer, rows the kernel may write).  The rows past them still hold the
    sentinel, bit for bit; the rows before them hold finite results and no sentinel."""
    for name, (full, rows) in bufs.items():
        live, guard = full[:rows], full[rows:]
        assert bool((guard == SENT).all()), \
            f"{what}: {name} written past row {rows} ({int((guard != SENT).sum())} elements of the guard rows)"
        assert bool(torch.isfinite(live).all()), f"{what}: {name} not finite"
        assert not bool((live == SENT).any()), \
            f"{what}: {name} has {int((live == SENT).sum())} elements never written in rows < {rows}"


def _normwise(name, got, ref):
    err = (got.double().cpu() - ref).norm().item()
    assert err <= 1e-4 * ref.norm().item() + 1e-6, f"{name}: {err:.3e} vs |ref| {ref.norm().item():.3e}"


def _dev(ts, device):
    return [t.float().to(device).contiguous() if t is not None else None for t in ts]


def _tail_forward(device, m, D):
    """The tail forward through the wrapper into guarded buffers; (device inputs, name -> (buffer, m))."""
    ins = _dev(_tail_case(m, D, True)[0], device)
    prev, agg, Wp, bp, gm, bt, Wm, bm = ins
    bufs = {n: _guarded(m, w, device) for n, w in (("view", D), ("x", D), ("h", D), ("rs", 2))}
    _native.view_chain_tail_fwd(prev, agg, Wp, bp, gm, bt, EPS, Wm, bm, *(bufs[n][1] for n in ("view", "x", "h", "rs")))
    return ins, {n: (full, m) for n, (full, _) in bufs.items()}


def _hub_forward(device, m, D, packed):
    ins = _dev(_hub_case(m, D, True)[0], device)
    v, gC, bC, Wv, Wl, bl, gA, bA, Wa, ba, Wr, br = ins
    bufs = {n: _guarded(m, w, device) for n, w in (("XL", D), ("t", 32), ("rs", 2))}
    if packed:  # SV | XR as the column halves of one [m + 16, 64] block, ldo = 64
        bufs["SV|XR"] = _guarded(m, 64, device)
        sv, xr = bufs["SV|XR"][1][:, :32], bufs["SV|XR"][1][:, 32:]
    else:
        bufs["SV"], bufs["XR"] = _guarded(m, 32, device), _guarded(m, 32, device)
        sv, xr = bufs["SV"][1], bufs["XR"][1]
    _native.view_chain_hub_fwd(v, EPS, Wl, bl, gC, bC, Wv, gA, bA, Wa, ba, Wr, br, bufs["XL"][1], sv, bufs["t"][1], xr,
                               bufs["rs"][1])
    outs = {"XL": bufs["XL"][1], "SV": sv, "XR": xr, "t": bufs["t"][1], "rs": bufs["rs"][1]}
    return ins, {n: (full, m) for n, (full, _) in bufs.items()}, outs


def _row_stats(x, D):
    mean = x.mean(1, keepdim=True)
    return torch.cat([mean, (x.var(1, unbiased=False, keepdim=True) + EPS).rsqrt()], 1)


@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=_ids(KERNEL_SHAPES))
def test_tail_fwd_guard_rows(device, shape):
    m, D = shape
    _, bufs = _tail_forward(device, m, D)
    _check_guards(bufs, "view_chain_tail_fwd")
    ins, _, _, y64 = _tail_case(m, D, True)
    prev, agg, Wp, bp, gm, bt, Wm, bm = ins
    x64 = F.linear(agg, Wp, bp) + prev
    refs = {"view": y64, "x": x64, "h": F.relu(F.layer_norm(x64, (D,), gm, bt, EPS)), "rs": _row_stats(x64, D)}
    _check([bufs[n][0][:m] for n in refs], list(refs.values()), list(refs))


@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=_ids(KERNEL_SHAPES))
@pytest.mark.parametrize("packed", [False, True])
def test_hub_fwd_guard_rows(device, shape, packed):
    m, D = shape
    _, bufs, outs = _hub_forward(device, m, D, packed)
    _check_guards(bufs, "view_chain_hub_fwd")
    ins, _, _, outs64 = _hub_case(m, D, True)
    v, gC, bC, Wv, Wl, bl, gA, bA, Wa, ba, Wr, br = ins
    refs = {"SV": outs64[1], "XL": outs64[2], "XR": outs64[3], "rs": _row_stats(v, D),
            "t": F.linear(F.relu(F.layer_norm(v, (D,), gA, bA, EPS)), Wa, ba)}
    _check([outs[n] for n in refs], list(refs.values()), list(refs))


def _tail_backward(device, m, D, ins, fwd, scratch=None, cnt=None):
    """The tail backward into fresh guarded buffers: through the wrapper, or (scratch, cnt given)
    through the C ABI with the caller's workspace and counters, in the wrapper's argument order."""
    prev, agg, Wp, bp, gm, bt, Wm, bm = ins
    x, h, rs = (fwd[n][0][:m] for n in ("x", "h", "rs"))
    dv = _tail_case(m, D, True)[1].float().to(device)
    T = (m + TR - 1) // TR
    bufs = {n: _guarded(m, w, device) for n, w in (("dh", D), ("dx", D), ("dagg", 32))}
    bufs["part"] = _guarded(T, _native.view_tail_part_cols(D), device, extra=1)
    dWm = _nan(D, device)
    outs = [bufs[n][1] for n in ("dh", "dx", "dagg", "part")]
    if scratch is None:
        _native.view_chain_tail_bwd(dv, x, h, rs, agg, Wp, gm, bt, Wm, outs[0], dWm, outs[1], outs[2], outs[3])
    else:
        p = _native._p
        st = _native.lib().gasfm_view_chain_tail_bwd(p(dv), p(x), p(h), p(rs), p(agg), m, D, p(Wp), p(gm), p(bt),
                                                     p(Wm), p(outs[0]), p(dWm), p(outs[1]), p(outs[2]), p(outs[3]),
                                                     p(scratch), p(cnt), _native._stream(x))
        _native.check(st, "gasfm_view_chain_tail_bwd")
    guards = {n: (full, m) for n, (full, _) in bufs.items()}
    guards["part"] = (bufs["part"][0], T)
    return guards, dWm


def _hub_backward(device, m, D, ins, outs, scratch=None):
    v, gC, bC, Wv, Wl, bl, gA, bA, Wa, ba, Wr, br = ins
    dskip, dsv, dxl, dxr = _dev(_hub_case(m, D, True)[1], device)
    T = (m + TR - 1) // TR
    bufs = {"dacc": _guarded(m, D, device), "part": _guarded(T, _native.view_hub_part_cols(D), device, extra=1)}
    dWl = _nan(D, device)
    dacc, part = bufs["dacc"][1], bufs["part"][1]
    rs, t = outs["rs"], outs["t"]
    if scratch is None:
        _native.view_chain_hub_bwd(v, rs, gC, bC, Wv, gA, bA, Wa, t, Wr, Wl, dsv, dxr, dxl, dskip, dacc, dWl, part)
    else:
        p = _native._p
        st = _native.lib().gasfm_view_chain_hub_bwd(p(v), p(rs), m, D, p(gC), p(bC), p(Wv), p(gA), p(bA), p(Wa), p(t),
                                                    p(Wr), p(Wl), p(dsv), p(dxr), p(dxl), p(dskip), p(dacc), p(dWl),
                                                    p(part), p(scratch), _native._stream(v))
        _native.check(st, "gasfm_view_chain_hub_bwd")
    return {"dacc": (bufs["dacc"][0], m), "part": (bufs["part"][0], T)}, dWl


@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=_ids(KERNEL_SHAPES))
def test_tail_bwd_guard_rows(device, shape):
    m, D = shape
    ins, fwd = _tail_forward(device, m, D)
    guards, dWm = _tail_backward(device, m, D, ins, fwd)
    _check_guards(guards, "view_chain_tail_bwd")
    assert bool(torch.isfinite(dWm).all()), "dWm not written in full"
    ref = _tail_case(m, D, True)[2]
    _normwise("d agg", guards["dagg"][0][:m], ref[1].grad)
    _normwise("dx", guards["dx"][0][:m], ref[0].grad)
    _normwise("dWm", dWm, ref[6].grad)


@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=_ids(KERNEL_SHAPES))
def test_hub_bwd_guard_rows(device, shape):
    m, D = shape
    ins, _, outs = _hub_forward(device, m, D, False)
    guards, dWl = _hub_backward(device, m, D, ins, outs)
    _check_guards(guards, "view_chain_hub_bwd")
    assert bool(torch.isfinite(dWl).all()), "dWl not written in full"
    ref = _hub_case(m, D, True)[2]
    _normwise("dv", guards["dacc"][0][:m], ref[0].grad)
    _normwise("dWl", dWl, ref[4].grad)


POISON = (float("nan"), 1e30, float("nan"))


@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=_ids(KERNEL_SHAPES))
def test_tail_bwd_poisoned_workspace(device, shape):
    """Nothing the backward reads from its workspace is left from an earlier call: NaN, 1e30 and NaN
    again in every scratch float give the same bits, and the tickets are back at zero each time."""
    m, D = shape
    ins, fwd = _tail_forward(device, m, D)
    ref = _tail_case(m, D, True)[2]
    L = _native.lib()
    scratch = torch.empty(int(L.gasfm_view_chain_scratch_floats(m, D)), dtype=torch.float32, device=device)
    cnt = torch.zeros(int(L.gasfm_view_chain_counters(m)), dtype=torch.int32, device=device)  # uint32 tickets
    runs = []
    for fill in POISON:
        scratch.fill_(fill)
        guards, dWm = _tail_backward(device, m, D, ins, fwd, scratch, cnt)
        assert not bool(cnt.any()), f"tickets after the call (scratch = {fill}): {cnt.tolist()}"
        _check_guards(guards, f"view_chain_tail_bwd, scratch = {fill}")
        assert bool(torch.isfinite(dWm).all()), f"dWm not finite (scratch = {fill})"
        _normwise("d agg", guards["dagg"][0][:m], ref[1].grad)
        _normwise("dx", guards["dx"][0][:m], ref[0].grad)
        runs.append([guards[n][0] for n in ("dx", "dagg", "dh", "part")] + [dWm])
    for other in runs[1:]:
        _same_bits(("dx", "dagg", "dh", "part", "dWm"), runs[0], other)


@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=_ids(KERNEL_SHAPES))
def test_hub_bwd_poisoned_workspace(device, shape):
    m, D = shape
    ins, _, outs = _hub_forward(device, m, D, False)
    ref = _hub_case(m, D, True)[2]
    L = _native.lib()
    scratch = torch.empty(int(L.gasfm_view_chain_scratch_floats(m, D)), dtype=torch.float32, device=device)
    runs = []
    for fill in POISON:
        scratch.fill_(fill)
        guards, dWl = _hub_backward(device, m, D, ins, outs, scratch)
        _check_guards(guards, f"view_chain_hub_bwd, scratch = {fill}")
        assert bool(torch.isfinite(dWl).all()), f"dWl not finite (scratch = {fill})"
        _normwise("dv", guards["dacc"][0][:m], ref[0].grad)
        runs.append([guards["dacc"][0], guards["part"][0], dWl])
    for other in runs[1:]:
        _same_bits(("dacc", "part", "dWl"), runs[0], other)

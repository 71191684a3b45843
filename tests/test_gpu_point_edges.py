"""Edges of the scene-point kernels (csrc/point_block.hip, csrc/point_head.hip): last-tile remainders,
workgroup edges, exact-size buffers, recycled partial rows and the entry points' documented contracts.

References and bars are those of test_gpu_point_block.py (fp64 _tail_ref / _hub_ref: outputs
2e-5 max|ref| + 1e-5, fused 5e-5; gradients normwise 1e-4 |ref| + 1e-6) and test_gpu_point_head.py
(_within: 10x aten-fp32's own deviation from fp64).  Row-shaped gradients (d prev, d agg, dp) meet
their bar a second time over the last tile's rows 16 ((N-1)//16) .. N-1 alone: one wrong row in
70 001 weighs 1/265 of the whole norm, over its own tile it cannot hide.  Every fp64-compared case
has its LayerNorm betas moved off the ReLU edge (relu_edge.off_relu_edge: the tail's on
x = prev + Wp agg + bp, then the hub's beta_A and beta_C on p, for the fused Function on the fp64 p of
the shifted tail), which is satisfiable only for small N: hence N <= 321 there.  The case builders
(tail_case, hub_case, fused_case) need no GPU.

Which (N, variant) reaches which mechanism -- what a removed case would uncover:

  remainder      A wave owns a 16-row tile; N % 16 = 1 .. 15 and 0 all run (N = 1 .. 33).  The backward
                 kernels mask rows in the C layout, row 4 (lane >> 4) + r: a remainder that is no multiple
                 of 4 (1-3, 5-7, 9-11, 13-15) cuts a lane group in two, where cl_mask, cl_load, cl_store
                 and the `live` test of cl_ln_relu_bwd must agree.  Loads past the last row are clamped
                 to a live row, so a dropped mask adds a finite duplicate row to a weight gradient: only
                 the comparison with fp64 sees it (section A), no NaN does.
  idle waves     A point-block workgroup is 4 waves (64 rows), a head workgroup 8 (128 rows).
                 N <= 48 / 112 leaves whole waves idle inside wg_reduce_ordered; N = 49 .. 64 (113 .. 128)
                 is the full workgroup; N = 63 / 64 / 65 and 127 / 128 / 129 are the edges.
  second         N = 65 (point block) and N = 129 (head): a last workgroup with one live wave holding
  workgroup      one row; N = 127 .. 129, 257, 321: 2 .. 6 workgroups, i.e. several partial rows.
  multi-tile     N = 70 001 (point block: 4 376 tiles, more than the resident waves) and N = 200 000
  loop,          (head): the only sizes at which a wave loops and fetch(t + nw) runs; compared bitwise
  prefetch       with the exact-size run, in guarded and poisoned buffers (section C).  The Function-level
                 determinism case (N = 50 000) runs the same loop.
  exact-size     Section C: every row tensor is the first N rows of an (N + 16)-row buffer.  Outputs start
  buffers        as one sentinel bit pattern: a guard row that changed was "written past row N", a row
                 below N still holding it was skipped.  Inputs end in 16 NaN rows: a read past row N that
                 reaches an MFMA gives NaN even under a zero mask.  The head writes out[c N + row]
                 ([4, N], exact by the wrapper's shape check): a store one column past N lands on column 0
                 of the next row, so pts3D[:, 0] and pts3D[:, N-1] are checked on their own, and row 3 == 1.
  partial rows   Section C: the per-workgroup partial rows are torch.empty in production and param_colsum
                 sums every slot; here they are pre-filled NaN, 1e30, NaN in three successive calls, so a
                 slot a kernel does not write shows whatever the allocator recycled.
  HC=false       Section D: gC = None (and bC .. bD, XR None) into point_hub_fwd / point_tail_hub_fwd,
                 reachable through the _native wrappers (a None is passed as a null pointer).
  aliasing       Section D: point_hub_bwd with dX the same storage as dRes (allowed: each element is read
                 and written by the same lane) at N = 21, 65, 130 and in the multi-tile loop at 70 001;
                 dX aliasing X / dSA / dXL / dXR and a misaligned agg / X are refused before any launch.
  other paths    Section B: the hub backward with unused outputs (None gradients), N = 0, expanded and
                 column-strided upstream gradients, run-to-run determinism of the tail, and distinct
                 eps / eps_h through the fused Function (equal values would hide a swap).
"""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from gasfm_amd import _native, point_block
from relu_edge import off_relu_edge
from test_gpu_point_block import EPS, _hub_ref, _rnd, _tail_ref
from test_gpu_point_head import _aten, _head, _within

pytestmark = pytest.mark.gpu

TAIL_NAMES = ("prev", "agg", "Wp", "bp", "gamma", "beta", "Wm", "bm")
HUB_NAMES = ("p", "gA", "bA", "WA", "WB", "bB", "gC", "bC", "WC", "bWC", "WD", "bD")
HUB_OUTS = ("skip", "SA", "XL", "XR")
SWEEP_N = list(range(1, 34)) + [47, 48, 49, 63, 64, 65, 127, 128, 129, 257, 321]
HEAD_N = list(range(1, 34)) + [63, 64, 65, 127, 128, 129, 255, 256, 257]
PATH_N = [21, 65]
KERNEL_N = [1, 5, 17, 63, 65, 130]
CONTRACT_N = [21, 65, 130]
BIG_BLOCK_N, BIG_HEAD_N = 70_001, 200_000


# ------------------------------------------------------------------------------ fp64 cases (CPU only)
def _tail_ref_eps(prev, agg, Wp, bp, g, b, Wm, bm, eps):
    """_tail_ref of test_gpu_point_block.py with eps as an argument."""
    x = F.linear(agg, Wp, bp)
    if prev is not None:
        x = prev + x
    return x + F.linear(F.relu(F.layer_norm(x, (64,), g, b, eps)), Wm, bm)


def _hub_ref_eps(p, gA, bA, WA, WB, bB, gC, bC, WC, bWC, WD, bD, eps):
    """_hub_ref of test_gpu_point_block.py with eps as an argument."""
    SA = F.linear(F.relu(F.layer_norm(p, (64,), gA, bA, eps)), WA)
    XL = F.linear(p, WB, bB)
    XR = F.linear(F.linear(F.relu(F.layer_norm(p, (64,), gC, bC, eps)), WC, bWC), WD, bD)
    return p, SA, XL, XR


def _tail_inputs(g, N, with_prev, small=False):
    """fp64 PointTailFn inputs, beta off the ReLU edge; small: rows of variance ~1e-3 (scale 0.03)."""
    if small:
        ins = [_rnd(g, N, 64, scale=0.03) if with_prev else None, _rnd(g, N, 32, scale=0.03),
               _rnd(g, 64, 32, scale=0.2), _rnd(g, 64, scale=0.003)]
    else:
        ins = [_rnd(g, N, 64, scale=2, shift=0.3) if with_prev else None, _rnd(g, N, 32),
               _rnd(g, 64, 32, scale=0.2), _rnd(g, 64, scale=0.1)]
    return ins + [_rnd(g, 64, scale=0.3, shift=1), _rnd(g, 64, scale=0.2), _rnd(g, 64, 64, scale=0.125),
                  _rnd(g, 64, scale=0.1)]


def _tail_off_edge(ins, eps):
    prev, agg, Wp, bp = ins[:4]
    x = F.linear(agg, Wp, bp) + (prev if prev is not None else 0)
    ins[5] = off_relu_edge(x, ins[4], ins[5], eps)
    return ins


def _hub_params(g):
    """fp64 (gA, bA, WA, WB, bB, gC, bC, WC, bWC, WD, bD)."""
    return [_rnd(g, 64, scale=0.3, shift=1), _rnd(g, 64, scale=0.2), _rnd(g, 32, 64, scale=0.125),
            _rnd(g, 64, 64, scale=0.125), _rnd(g, 64, scale=0.1), _rnd(g, 64, scale=0.3, shift=1),
            _rnd(g, 64, scale=0.2), _rnd(g, 32, 64, scale=0.125), _rnd(g, 32, scale=0.1),
            _rnd(g, 32, 32, scale=0.18), _rnd(g, 32, scale=0.1)]


def _hub_off_edge(p, prm, eps):
    prm[1], prm[6] = off_relu_edge(p, prm[0], prm[1], eps), off_relu_edge(p, prm[5], prm[6], eps)
    return prm


def _leaves(ts):
    return [t.clone().requires_grad_(True) if t is not None else None for t in ts]


@functools.lru_cache(maxsize=None)
def tail_case(N, with_prev):
    """(fp64 inputs, dout, the fp64 leaves holding their .grad, the fp64 output); shared, never modified."""
    g = torch.Generator().manual_seed(1000 + 2 * N + with_prev)
    ins = _tail_off_edge(_tail_inputs(g, N, with_prev), EPS)
    dout = _rnd(g, N, 64)
    ref = _leaves(ins)
    y64 = _tail_ref(*ref)
    y64.backward(dout)
    return ins, dout, ref, y64.detach()


@functools.lru_cache(maxsize=None)
def hub_case(N, used=(0, 1, 2, 3)):
    """(fp64 inputs, the gradients of (skip, SA, XL, XR), None where not in ``used``, the fp64 leaves holding
    their .grad (None for a parameter no used output depends on), the fp64 outputs)."""
    g = torch.Generator().manual_seed(2000 + N)  # the same inputs for every ``used``
    p = _rnd(g, N, 64, scale=1.5, shift=-0.2)
    ins = [p] + _hub_off_edge(p, _hub_params(g), EPS)
    grads = [_rnd(g, N, 64), _rnd(g, N, 32), _rnd(g, N, 64), _rnd(g, N, 32)]
    grads = [d if k in used else None for k, d in enumerate(grads)]
    ref = _leaves(ins)
    outs64 = _hub_ref(*ref)
    torch.autograd.backward([o for o, d in zip(outs64, grads) if d is not None], [d for d in grads if d is not None])
    return ins, grads, ref, [o.detach() for o in outs64]


@functools.lru_cache(maxsize=None)
def fused_case(N, with_prev, eps=EPS, eps_h=EPS, small=False):
    """(fp64 tail inputs, fp64 hub parameters, gradients of (p, SA, XL, XR), the fp64 leaves holding their
    .grad, the fp64 outputs) of PointTailHubFn."""
    g = torch.Generator().manual_seed(3000 + 2 * N + with_prev + 7 * small)
    t_in = _tail_off_edge(_tail_inputs(g, N, with_prev, small), eps)
    h_in = _hub_off_edge(_tail_ref_eps(*t_in, eps), _hub_params(g), eps_h)
    grads = [_rnd(g, N, 64), _rnd(g, N, 32), _rnd(g, N, 64), _rnd(g, N, 32)]
    r_t, r_h = _leaves(t_in), _leaves(h_in)
    outs64 = _hub_ref_eps(_tail_ref_eps(*r_t, eps), *r_h, eps_h)
    torch.autograd.backward(list(outs64), grads)
    return t_in, h_in, grads, r_t + r_h, [o.detach() for o in outs64]


def all_case_builders():
    """Every fp64 case of this file, built (each builder asserts its ReLU margin); needs no GPU."""
    n = 0
    for N in SWEEP_N:
        for flag in (True, False):
            tail_case(N, flag), fused_case(N, flag)
            n += 2
        hub_case(N)
        n += 1
    for N in PATH_N:
        for used in HUB_SUBSETS:
            hub_case(N, used)
        for flag in (True, False):
            fused_case(N, flag, 1e-5, 1e-3, True)
        n += len(HUB_SUBSETS) + 2
    for N in CONTRACT_N:
        hub_case(N), fused_case(N, True), fused_case(N, False)
        n += 3
    return n


# ------------------------------------------------------------------------------ comparisons
def _dev(ts, device):
    return [t.float().to(device).requires_grad_(True) if t is not None else None for t in ts]


def _close_outs(names, outs, refs, rel=2e-5):
    for name, o, r in zip(names, outs, refs):
        torch.testing.assert_close(o.double().cpu(), r, rtol=0, atol=rel * r.abs().max().item() + 1e-5, msg=name)


def _close_grads(names, got, ref):
    """_close_grads of test_gpu_point_block.py; a parameter no used output depends on has the gradient 0."""
    for name, a, r in zip(names, got, ref):
        if r is None:
            continue
        ga, gr = a.grad.double().cpu(), r.grad if r.grad is not None else torch.zeros_like(r)
        err = (ga - gr).norm().item()
        assert err <= 1e-4 * gr.norm().item() + 1e-6, f"{name}: {err:.3e} vs |ref| {gr.norm().item():.3e}"


def _close_last_tile(names, got, ref, N):
    """The gradient bar over the last tile's rows alone, for the row-shaped gradients."""
    lo = 16 * ((N - 1) // 16)
    for name, a, r in zip(names, got, ref):
        if r is None or name not in ("prev", "agg", "p"):
            continue
        ga, gr = a.grad.double().cpu()[lo:], r.grad[lo:]
        err = (ga - gr).norm().item()
        assert err <= 1e-4 * gr.norm().item() + 1e-6, \
            f"{name} rows {lo}..{N - 1}: {err:.3e} vs |ref| {gr.norm().item():.3e}"


def _run_tail(device, N, with_prev):
    ins, dout, ref, y64 = tail_case(N, with_prev)
    got = _dev(ins, device)
    y = point_block.PointTailFn.apply(*got, EPS)
    y.backward(dout.float().to(device))
    _close_outs(["out"], [y], [y64])
    _close_grads(TAIL_NAMES, got, ref)
    _close_last_tile(TAIL_NAMES, got, ref, N)


def _run_hub(device, N, used):
    ins, grads, ref, outs64 = hub_case(N, used)
    got = _dev(ins, device)
    outs = point_block.PointHubFn.apply(*got, EPS)
    _close_outs(HUB_OUTS, outs, outs64)
    torch.autograd.backward([o for o, d in zip(outs, grads) if d is not None],
                            [d.float().to(device) for d in grads if d is not None])
    _close_grads(HUB_NAMES, got, ref)
    _close_last_tile(HUB_NAMES, got, ref, N)
    return got, ref


def _run_fused(device, case, eps, eps_h, N):
    t_in, h_in, grads, ref, outs64 = case
    got = _dev(t_in, device) + _dev(h_in, device)
    outs = point_block.PointTailHubFn.apply(*got[:8], eps, *got[8:], eps_h)
    _close_outs(("p",) + HUB_OUTS[1:], outs, outs64, rel=5e-5)
    torch.autograd.backward(outs, [d.float().to(device) for d in grads])
    _close_grads(TAIL_NAMES + HUB_NAMES[1:], got, ref)
    _close_last_tile(TAIL_NAMES + HUB_NAMES[1:], got, ref, N)
    return outs, got


# ------------------------------------------------------------------------------ A. remainder / workgroup sweep
@pytest.mark.parametrize("N", SWEEP_N)
@pytest.mark.parametrize("with_prev", [True, False])
def test_a_tail_sweep(device, N, with_prev):
    _run_tail(device, N, with_prev)


@pytest.mark.parametrize("N", SWEEP_N)
@pytest.mark.parametrize("with_skip", [True, False])
def test_a_hub_sweep(device, N, with_skip):
    _run_hub(device, N, (0, 1, 2, 3) if with_skip else (1, 2, 3))


@pytest.mark.parametrize("N", SWEEP_N)
@pytest.mark.parametrize("with_prev", [True, False])
def test_a_tail_hub_sweep(device, N, with_prev):
    _run_fused(device, fused_case(N, with_prev), EPS, EPS, N)


@pytest.mark.parametrize("N", HEAD_N)
def test_a_head_sweep(device, N):
    seq = _head(N, device)
    g = torch.Generator(device="cpu").manual_seed(N + 1)
    p = torch.randn(N, 64, generator=g).to(device)
    dout = torch.randn(4, N, generator=g).to(device)
    assert point_block.head_fusable(seq, p)

    def run(fn, s, x):
        x = x.clone().requires_grad_(True)
        for prm in s.parameters():
            prm.grad = None
        y = fn(s, x)
        y.backward(dout.to(x.dtype))
        return [y.detach(), x.grad] + [prm.grad.clone() for prm in s.parameters()]

    ours = run(point_block.head, seq, p)
    aten = run(_aten, seq, p)
    seq64 = _head(N, device).double()
    seq64.load_state_dict({k: v.double() for k, v in seq.state_dict().items()})
    ref = run(_aten, seq64, p.double())
    names = ["pts3D", "dp"] + [n for n, _ in seq.named_parameters()]
    for o, a, r, name in zip(ours, aten, ref, names):
        assert o.shape == r.shape, name
        _within(o, a, r, name)
    lo = 16 * ((N - 1) // 16)
    _within(ours[1][lo:], aten[1][lo:], ref[1][lo:], f"dp rows {lo}..{N - 1}")
    assert bool((ours[0][3] == 1).all()), "pts3D[3] is not exactly 1"
    for col in (0, N - 1):
        _within(ours[0][:3, col], aten[0][:3, col], ref[0][:3, col], f"pts3D[:, {col}]")


# ------------------------------------------------------------------------------ B. paths nobody runs
HUB_SUBSETS = [(1,), (2,), (3,), (0,), (1, 3)]


@pytest.mark.parametrize("N", PATH_N)
@pytest.mark.parametrize("used", HUB_SUBSETS, ids=lambda u: "+".join(HUB_OUTS[k] for k in u))
def test_b_hub_unused_outputs(device, N, used):
    """dSA / dXL / dXR = None in _hub_backward (set_materialize_grads(False)): every parameter gradient
    matches fp64, and those of a branch no used output depends on are exactly 0."""
    got, ref = _run_hub(device, N, used)
    for name, a, r in zip(HUB_NAMES, got, ref):
        assert a.grad is not None and a.grad.shape == a.shape, name
        if r.grad is None:
            assert int(torch.count_nonzero(a.grad)) == 0, f"{name}: not exactly 0 with its branch unused"
    if 2 not in used:
        assert int(torch.count_nonzero(got[4].grad)) == 0 and int(torch.count_nonzero(got[5].grad)) == 0, "dWB / dbB"


def test_b_empty(device):
    """N = 0 through the three Functions: shapes, zero parameter gradients, and no launch -- the C entry
    points return OK at N = 0 before they look at a pointer, shown by passing none."""
    before = _native.lib().gasfm_last_error()
    g = torch.Generator().manual_seed(9)
    for with_prev in (True, False):
        t_in, h_in = _tail_inputs(g, 0, with_prev), _hub_params(g)
        runs = [(point_block.PointTailFn, _dev(t_in, device), (EPS,), [(0, 64)]),
                (point_block.PointHubFn, _dev([_rnd(g, 0, 64)] + h_in, device), (EPS,),
                 [(0, 64), (0, 32), (0, 64), (0, 32)])]
        for fn, leaves, tail_args, shapes in runs:
            outs = fn.apply(*leaves, *tail_args)
            outs = outs if isinstance(outs, tuple) else (outs,)
            assert [tuple(o.shape) for o in outs] == shapes, fn.__name__
            sum(o.sum() for o in outs).backward()
            for t in leaves:
                if t is not None:
                    assert t.grad is not None and t.grad.shape == t.shape, fn.__name__
                    assert int(torch.count_nonzero(t.grad)) == 0, fn.__name__
        leaves = _dev(t_in, device) + _dev(h_in, device)
        outs = point_block.PointTailHubFn.apply(*leaves[:8], EPS, *leaves[8:], EPS)
        assert [tuple(o.shape) for o in outs] == [(0, 64), (0, 32), (0, 64), (0, 32)]
        sum(o.sum() for o in outs).backward()
        for t in leaves:
            if t is not None:
                assert t.grad is not None and t.grad.shape == t.shape and int(torch.count_nonzero(t.grad)) == 0
    L, nul, eps = _native.lib(), None, ctypes.c_float(EPS)
    assert L.gasfm_point_tail_fwd(*[nul] * 2, 0, *[nul] * 4, eps, *[nul] * 4) == 0
    assert L.gasfm_point_tail_bwd(*[nul] * 3, 0, *[nul] * 4, eps, *[nul] * 5) == 0
    assert L.gasfm_point_hub_fwd(nul, 0, eps, *[nul] * 15) == 0
    assert L.gasfm_point_tail_hub_fwd(*[nul] * 2, 0, *[nul] * 4, eps, *[nul] * 3, eps, *[nul] * 15) == 0
    assert L.gasfm_point_hub_bwd(nul, 0, eps, *[nul] * 17) == 0
    for has in (0, 1):
        assert _native.point_tail_part_shape(0, has)[0] == 0 and _native.point_hub_part_shape(0, has, has)[0] == 0
    torch.cuda.synchronize()
    assert _native.lib().gasfm_last_error() == before


def _grads_of(leaves):
    return [t.grad.clone() for t in leaves if t is not None]


@pytest.mark.parametrize("N", PATH_N)
@pytest.mark.parametrize("fn", ["tail", "hub", "tail_hub"])
def test_b_noncontiguous_upstream(device, N, fn):
    """Expanded (stride-0, out.sum().backward()) and column-strided (big[:, ::2]) upstream gradients give
    bitwise the gradients of their contiguous copies."""
    g = torch.Generator().manual_seed(40 + N)
    if fn == "tail":
        ins, apply = _tail_inputs(g, N, True), lambda x: (point_block.PointTailFn.apply(*x, EPS),)
    elif fn == "hub":
        ins, apply = [_rnd(g, N, 64)] + _hub_params(g), lambda x: point_block.PointHubFn.apply(*x, EPS)
    else:
        ins = _tail_inputs(g, N, True) + _hub_params(g)
        apply = lambda x: point_block.PointTailHubFn.apply(*x[:8], EPS, *x[8:], EPS)  # noqa: E731

    def grads(upstream):
        leaves = _dev(ins, device)
        outs = apply(leaves)
        if upstream is None:
            sum(o.sum() for o in outs).backward()
        else:
            torch.autograd.backward(outs, upstream(outs))
        return _grads_of(leaves)

    big = [torch.randn(N, 2 * (32 if k in (1, 3) else 64), generator=g).to(device) for k in range(4)]
    if fn == "tail":
        big = big[:1]
    strided = [b[:, ::2] for b in big]
    assert not any(s.is_contiguous() for s in strided)
    for a, b in ((grads(None), grads(lambda outs: [torch.ones_like(o) for o in outs])),
                 (grads(lambda outs: strided), grads(lambda outs: [s.contiguous() for s in strided]))):
        for x, y in zip(a, b):
            assert torch.equal(x, y)


@pytest.mark.parametrize("with_prev", [True, False])
def test_b_tail_deterministic(device, with_prev):
    g = torch.Generator().manual_seed(6)
    ins = _dev(_tail_inputs(g, 50_000, with_prev), device)
    dout = _rnd(g, 50_000, 64).float().to(device)
    res = []
    for _ in range(2):
        for t in ins:
            if t is not None:
                t.grad = None
        y = point_block.PointTailFn.apply(*ins, EPS)
        y.backward(dout)
        res.append([y.detach().clone()] + _grads_of(ins))
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.mark.parametrize("N", PATH_N)
@pytest.mark.parametrize("with_prev", [True, False])
def test_b_fused_eps_pair(device, N, with_prev):
    """Distinct eps (tail) and eps_h (hub) through PointTailHubFn, on rows of small variance."""
    eps, eps_h = 1e-5, 1e-3
    case = fused_case(N, with_prev, eps, eps_h, True)
    t_in, h_in, grads, _, outs64 = case
    # the case can see a swap: the fp64 outputs with the two values exchanged leave the bar 100 times over
    swapped = _hub_ref_eps(_tail_ref_eps(*t_in, eps_h), *h_in, eps)
    for name, s, r in zip(("p",) + HUB_OUTS[1:], swapped, outs64):
        bar = 5e-5 * r.abs().max().item() + 1e-5
        assert (s - r).abs().max().item() > 100 * bar, f"{name}: a swapped eps pair would pass"
    outs1, got1 = _run_fused(device, case, eps, eps_h, N)
    got2 = _dev(t_in, device) + _dev(h_in, device)
    outs2 = point_block.PointHubFn.apply(point_block.PointTailFn.apply(*got2[:8], eps), *got2[8:], eps_h)
    torch.autograd.backward(outs2, [d.float().to(device) for d in grads])
    for name, a, b in zip(("p",) + HUB_OUTS[1:], outs1, outs2):
        assert torch.equal(a, b), name
    for name, a, b in zip(TAIL_NAMES + HUB_NAMES[1:], got1, got2):
        if a is not None:
            assert torch.equal(a.grad, b.grad), name


# ------------------------------------------------------------------------------ C. kernel level
GUARD, PART_GUARD = 16, 2
SENTINEL = 0x7FC5A5A5  # a NaN payload no arithmetic produces


def _weights(device):
    g = torch.Generator().manual_seed(77)
    t_in, h_in = _tail_inputs(g, 1, False), _hub_params(g)
    w = dict(zip(TAIL_NAMES[2:], t_in[2:]))
    w.update(zip(HUB_NAMES[1:], h_in))
    w.update(W1=_rnd(g, 64, 64, scale=0.125), b1=_rnd(g, 64, scale=0.1), W2=_rnd(g, 64, 64, scale=0.125),
             b2=_rnd(g, 64, scale=0.1), W3=_rnd(g, 3, 64, scale=0.125), b3=_rnd(g, 3, scale=0.1))
    return {k: v.float().to(device) for k, v in w.items()}


class Entry:
    """One _native.point_* entry point: its row inputs / outputs {name: width}, exact-shape tensors
    {name: shape(N)}, partial buffers {name: shape(N)} and the call on a dict of all of them."""

    def __init__(self, name, ins, outs, call, parts=None, exact_in=None, exact_out=None, head=False):
        self.name, self.ins, self.outs, self.call, self.head = name, ins, outs, call, head
        self.parts, self.exact_in, self.exact_out = parts or {}, exact_in or {}, exact_out or {}


def _tail_fwd(w, t):
    _native.point_tail_fwd(t.get("prev"), t["agg"], w["Wp"], w["bp"], w["gamma"], w["beta"], EPS, w["Wm"], w["bm"],
                           t["out"])


def _tail_bwd(w, t):
    _native.point_tail_bwd(t["dout"], t.get("prev"), t["agg"], w["Wp"], w["bp"], w["gamma"], w["beta"], EPS, w["Wm"],
                           t["dx"], t["dagg"], t["part"])


def _hub_fwd(w, t, hc=True):
    c = [w[k] if hc else None for k in ("gC", "bC", "WC", "bWC", "WD", "bD")]
    _native.point_hub_fwd(t["X"], EPS, w["gA"], w["bA"], w["WA"], t["SA"], w["WB"], w["bB"], t["XL"], *c,
                          t["XR"] if hc else None)


def _tail_hub_fwd(w, t, hc=True):
    c = [w[k] if hc else None for k in ("gC", "bC", "WC", "bWC", "WD", "bD")]
    _native.point_tail_hub_fwd(t.get("prev"), t["agg"], w["Wp"], w["bp"], w["gamma"], w["beta"], EPS, w["Wm"],
                               w["bm"], t["p"], EPS, w["gA"], w["bA"], w["WA"], t["SA"], w["WB"], w["bB"], t["XL"],
                               *c, t["XR"] if hc else None)


def _hub_bwd(w, t):
    _native.point_hub_bwd(t["X"], EPS, w["gA"], w["bA"], w["WA"], w["WB"], w["gC"], w["bC"], w["WC"], w["bWC"],
                          w["WD"], t["dSA"], t["dXL"], t["dXR"], t.get("dRes"), t["dX"], t["part_a"], t["part_c"])


def _head_fwd(w, t):
    _native.point_head_fwd(t["P"], w["W1"], w["b1"], w["W2"], w["b2"], w["W3"], w["b3"], t["out"])


def _head_bwd(w, t):
    _native.point_head_bwd(t["P"], w["W1"], w["b1"], w["W2"], w["b2"], w["W3"], t["dout"], t["dP"], t["part_a"],
                           t["part_b"])


def _with(d, flag, **extra):
    return dict(d, **extra) if flag else d


ENTRIES = {}
for _f in (True, False):
    _s = "prev" if _f else "noprev"
    ENTRIES[f"tail_fwd-{_s}"] = Entry("tail_fwd", _with({"agg": 32}, _f, prev=64), {"out": 64}, _tail_fwd)
    ENTRIES[f"tail_bwd-{_s}"] = Entry(
        "tail_bwd", _with({"dout": 64, "agg": 32}, _f, prev=64), {"dx": 64, "dagg": 32}, _tail_bwd,
        parts={"part": lambda N, f=_f: _native.point_tail_part_shape(N, f)})
    ENTRIES[f"tail_hub_fwd-{_s}"] = Entry("tail_hub_fwd", _with({"agg": 32}, _f, prev=64),
                                          {"p": 64, "SA": 32, "XL": 64, "XR": 32}, _tail_hub_fwd)
    _s = "dres" if _f else "nodres"
    ENTRIES[f"hub_bwd-{_s}"] = Entry(
        "hub_bwd", _with({"X": 64, "dSA": 32, "dXL": 64, "dXR": 32}, _f, dRes=64), {"dX": 64}, _hub_bwd,
        parts={"part_a": lambda N: _native.point_hub_part_shape(N, 0, True),
               "part_c": lambda N, f=_f: _native.point_hub_part_shape(N, 1, f)})
ENTRIES["hub_fwd"] = Entry("hub_fwd", {"X": 64}, {"SA": 32, "XL": 64, "XR": 32}, _hub_fwd)
ENTRIES["head_fwd"] = Entry("head_fwd", {"P": 64}, {}, _head_fwd, exact_out={"out": lambda N: (4, N)}, head=True)
ENTRIES["head_bwd"] = Entry("head_bwd", {"P": 64}, {"dP": 64}, _head_bwd, exact_in={"dout": lambda N: (4, N)},
                            parts={"part_a": lambda N: _native.point_head_part_shape(N, 0),
                                   "part_b": lambda N: _native.point_head_part_shape(N, 1)}, head=True)
BLOCK_ENTRIES = [k for k, e in ENTRIES.items() if not e.head]
HEAD_ENTRIES = [k for k, e in ENTRIES.items() if e.head]


def _bits(t):
    return t.view(torch.int32)


def _sentinel(shape, device):
    return torch.full(shape, SENTINEL, dtype=torch.int32, device=device).view(torch.float32)


def _inputs(entry, N, device):
    g = torch.Generator().manual_seed(500 + N)
    t = {k: torch.randn(N, w, generator=g).to(device) for k, w in entry.ins.items()}
    t.update({k: torch.randn(*shape(N), generator=g).to(device) for k, shape in entry.exact_in.items()})
    return t


def _run_plain(entry, w, ins, N, device):
    """The call on exact-size, unpoisoned buffers: {output or partial name: tensor}."""
    res = {k: torch.empty(N, wd, device=device) for k, wd in entry.outs.items()}
    res.update({k: torch.empty(shape(N), device=device) for k, shape in entry.exact_out.items()})
    res.update({k: torch.empty(shape(N), device=device) for k, shape in entry.parts.items()})
    entry.call(w, dict(ins, **res))
    return res


def _run_guarded(entry, w, ins, N, device, part_fill=float("nan")):
    """The call with every row tensor the first N rows of an (N + 16)-row buffer: inputs followed by NaN
    rows, outputs pre-filled with the sentinel, partials pre-filled with part_fill and followed by 2
    guard rows.  Checks the guards, that every element below them was written, and that every result
    (and the partials' column sums) is finite; returns {output or partial name: tensor}."""
    t, bufs = dict(ins), {}
    for k, wd in entry.ins.items():
        big = torch.full((N + GUARD, wd), float("nan"), device=device)
        big[:N] = ins[k]
        t[k] = big[:N]
    for k, wd in entry.outs.items():
        bufs[k] = _sentinel((N + GUARD, wd), device)
        t[k] = bufs[k][:N]
    for k, shape in entry.exact_out.items():
        t[k] = _sentinel(shape(N), device)
    for k, shape in entry.parts.items():
        rows, cols = shape(N)
        bufs[k] = torch.full((rows + PART_GUARD, cols), part_fill, device=device)
        t[k] = bufs[k][:rows]
    before = {k: _bits(b).clone() for k, b in bufs.items()}
    entry.call(w, t)
    res = {}
    for k in list(entry.outs) + list(entry.exact_out) + list(entry.parts):
        rows = t[k].shape[0]
        if k in bufs:
            assert torch.equal(_bits(bufs[k])[rows:], before[k][rows:]), f"{entry.name}: {k} written past row {rows}"
        if k not in entry.parts:
            assert not bool((_bits(t[k]) == SENTINEL).any()), f"{entry.name}: {k} has unwritten elements"
        assert bool(torch.isfinite(t[k]).all()), f"{entry.name}: {k} not finite"
        if k in entry.parts:
            assert bool(torch.isfinite(t[k].sum(0)).all()), f"{entry.name}: column sums of {k} not finite"
        res[k] = t[k].clone()
    if "out" in entry.exact_out:
        assert bool((res["out"][3] == 1).all()), "pts3D[3] is not exactly 1"
    return res


def _guard_rows(entry, N, device):
    w, ins = _weights(device), _inputs(entry, N, device)
    first = None
    for fill in (float("nan"), 1e30, float("nan")):
        res = _run_guarded(entry, w, ins, N, device, fill)
        first = first or res
        for k, v in res.items():
            assert torch.equal(_bits(v), _bits(first[k])), f"{entry.name}: {k} depends on what its buffer held"


def _equals_exact_size(entry, N, device):
    w, ins = _weights(device), _inputs(entry, N, device)
    plain, guarded = _run_plain(entry, w, ins, N, device), _run_guarded(entry, w, ins, N, device)
    for k, v in guarded.items():
        assert torch.equal(_bits(v), _bits(plain[k])), f"{entry.name}: {k} differs from the exact-size run"


@pytest.mark.parametrize("N", KERNEL_N)
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_c_guard_rows(device, entry, N):
    """Guard rows intact, every output element written, poisoned input tails never read, poisoned
    partial rows fully overwritten (NaN, 1e30, NaN in three successive calls).  Uses no exact-size
    output buffer: an out-of-range store lands in the test's own guard rows."""
    _guard_rows(ENTRIES[entry], N, device)


@pytest.mark.parametrize("N", KERNEL_N)
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_c_equals_exact_size(device, entry, N):
    _equals_exact_size(ENTRIES[entry], N, device)


@pytest.mark.parametrize("entry,N", [(e, BIG_BLOCK_N) for e in BLOCK_ENTRIES] + [(e, BIG_HEAD_N) for e in HEAD_ENTRIES])
def test_c_multi_tile(device, entry, N):
    """The sizes at which a wave loops over several tiles and the one-tile-ahead prefetch runs."""
    _guard_rows(ENTRIES[entry], N, device)
    _equals_exact_size(ENTRIES[entry], N, device)


# ------------------------------------------------------------------------------ D. contracts of the C entry points
def _f32(ts, device):
    return [t.float().to(device) if t is not None else None for t in ts]


@pytest.mark.parametrize("N", CONTRACT_N)
@pytest.mark.parametrize("fn", ["hub", "tail_hub-prev", "tail_hub-noprev"])
def test_d_no_c_branch(device, N, fn):
    """gC = None (bC .. bD, XR None): the HC=false kernels.  SA, XL (and p) within the output bar of fp64,
    the call OK, the guard rows of SA / XL / p intact."""
    if fn == "hub":
        ins, _, _, outs64 = hub_case(N)
        rows, prm, rel = {"X": ins[0]}, ins[1:], 2e-5
        call, names = _hub_fwd, ("SA", "XL")
    else:
        t_in, h_in, _, _, outs64 = fused_case(N, fn.endswith("-prev"))
        rows, prm, rel = {"agg": t_in[1]}, h_in, 5e-5
        if t_in[0] is not None:
            rows["prev"] = t_in[0]
        call, names = _tail_hub_fwd, ("p", "SA", "XL")
    w = dict(zip(HUB_NAMES[1:], _f32(prm, device)))
    if fn != "hub":
        w.update(zip(TAIL_NAMES[2:], _f32(t_in[2:], device)))
    t = {k: v.float().to(device) for k, v in rows.items()}
    bufs = {k: _sentinel((N + GUARD, 32 if k == "SA" else 64), device) for k in names}
    t.update({k: b[:N] for k, b in bufs.items()})
    call(w, t, hc=False)  # raises unless the entry point returns OK
    for k, b in bufs.items():
        assert bool((_bits(b)[N:] == SENTINEL).all()), f"{k} written past row {N}"
        assert not bool((_bits(b)[:N] == SENTINEL).any()), f"{k} has unwritten elements"
    ref = dict(zip(("p",) + HUB_OUTS[1:], outs64))
    _close_outs(names, [t[k] for k in names], [ref[k] for k in names], rel=rel)


def _hub_bwd_tensors(N, device, seed=0):
    g = torch.Generator().manual_seed(800 + N + seed)
    t = {k: torch.randn(N, wd, generator=g).to(device)
         for k, wd in (("X", 64), ("dSA", 32), ("dXL", 64), ("dXR", 32), ("dRes", 64))}
    for k, which in (("part_a", 0), ("part_c", 1)):
        t[k] = torch.full(_native.point_hub_part_shape(N, which, True), float("nan"), device=device)
    return t


@pytest.mark.parametrize("N", CONTRACT_N + [BIG_BLOCK_N])
def test_d_hub_bwd_dx_aliases_dres(device, N):
    """include/gasfm.h: dRes may alias dX.  dX and both partials bitwise equal to the non-aliased call."""
    w = _weights(device)
    plain = _hub_bwd_tensors(N, device)
    plain["dX"] = torch.empty(N, 64, device=device)
    _hub_bwd(w, plain)
    alias = _hub_bwd_tensors(N, device)
    alias["dX"] = alias["dRes"]
    assert alias["dX"].data_ptr() == alias["dRes"].data_ptr()
    _hub_bwd(w, alias)
    for k in ("dX", "part_a", "part_c"):
        assert bool(torch.isfinite(alias[k]).all()), k
        assert torch.equal(alias[k], plain[k]), k


@pytest.mark.parametrize("N", CONTRACT_N)
def test_d_refusals(device, N):
    """dX aliasing X, dSA, dXL or dXR, and a misaligned agg / X, raise before any launch: nothing the
    call could have written changes.  (Buffers are sized so that a launch, were the refusal missing,
    would still stay inside them.)"""
    w = _weights(device)
    for name in ("X", "dSA", "dXL", "dXR"):
        t = _hub_bwd_tensors(N, device)
        wd = t[name].shape[1]
        store = torch.zeros(N * 64, device=device)  # room for a [N, 64] dX whatever the input's width
        store[:N * wd] = t[name].reshape(-1)
        t[name] = store[:N * wd].view(N, wd)
        t["dX"] = t[name]
        keep = store.clone()
        with pytest.raises(RuntimeError, match="aliases"):
            _hub_bwd(w, t)
        torch.cuda.synchronize()
        assert torch.equal(store, keep) and bool(torch.isnan(t["part_a"]).all() and torch.isnan(t["part_c"]).all())

    def misaligned(wd):  # contiguous (what _req asks for), starting 4 bytes into its buffer
        flat = torch.randn(N * wd + 4, device=device)
        v = flat.as_strided((N, wd), (wd, 1), 1)
        assert v.is_contiguous() and v.data_ptr() % 16 == 4
        return v

    outs = {k: _sentinel((N + GUARD, wd), device)
            for k, wd in (("out", 64), ("p", 64), ("SA", 32), ("XL", 64), ("XR", 32), ("dx", 64), ("dagg", 32),
                          ("dX", 64))}
    part = _sentinel(_native.point_tail_part_shape(N, False), device)
    t = {k: b[:N] for k, b in outs.items()}
    t.update(_hub_bwd_tensors(N, device), part=part, dout=torch.randn(N, 64, device=device))
    for call, key in ((_tail_fwd, "agg"), (_tail_bwd, "agg"), (_tail_hub_fwd, "agg"), (_hub_fwd, "X"), (_hub_bwd, "X")):
        with pytest.raises(RuntimeError, match="alignment"):
            call(w, dict(t, **{key: misaligned(32 if key == "agg" else 64)}))
    torch.cuda.synchronize()
    for k, b in outs.items():
        assert bool((_bits(b) == SENTINEL).all()), f"{k} written by a refused call"
    assert bool((_bits(part) == SENTINEL).all()) and bool(torch.isnan(t["part_a"]).all())

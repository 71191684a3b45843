"""DepthHeadFn (csrc/depth_head.hip) against the depth head as the reference runs it
(code/models/graph_attn_sfm.py:153-162: depths = depth_head(P), the head Linear(128,128) ReLU
Linear(128,128) ReLU Linear(128,1), layers.py:10-44 norm=False, no ReLU before the first layer).

1. Parity.  Reference values: the same sequence in fp64.  Tolerance: the bound of
   test_gpu_point_head.py -- each result within 10x the fp32 aten result's own deviation from fp64,
   plus 1e-6 of the result's scale.  Sizes: tile remainders (15, 16, 17), the 48 rows of one
   workgroup pass (63, 64, 65 straddle the second), the 384 rows a backward workgroup is given
   before another one is added (383, 384, 385), several workgroups with a remainder (1000, 40,013).
   Every 7th row of P drives the whole first hidden vector negative (an all-zero ReLU mask: the row's
   second hidden vector is then b2 and its dP exactly zero); every third dd is zero.
2. Guards.  The guard-row / poison method of test_gpu_point_edges.py section C at the C entry points.
3. Memory, the point of the feature: the fused forward + backward allocates less than 2x the bytes of
   P beyond the resident inputs (dP, d, dd, the partial rows), aten more than 3x (y1, y2 and their
   gradients); and a captured replay reproduces the eager run bitwise.
"""
import pytest
import torch

from gasfm_amd import _native, depth_head
from gasfm_amd.depth_head import _binding
from gasfm_amd.model import get_linear_layers

pytestmark = pytest.mark.gpu

W = 128
ROWS_PER_WG = 384  # csrc/depth_head.hip: kWavesD * kMinTiles * 16 rows before the backward grid grows
SIZES = [1, 15, 16, 17, 63, 64, 65, ROWS_PER_WG - 1, ROWS_PER_WG, ROWS_PER_WG + 1, 1000, 40_013]
NAMES = ["d", "dP"] + [f"{i}.{k}" for i in (0, 2, 4) for k in ("weight", "bias")]


def _head(seed, device, dtype=torch.float32):
    torch.manual_seed(seed)
    return get_linear_layers(3 * [W] + [1], norm=False).to(device=device, dtype=dtype)


def _inputs(E, device, seed=None):
    """Random P [E, 128] and dd [E, 1] with every third dd zero."""
    g = torch.Generator(device="cpu").manual_seed(E + 1 if seed is None else seed)
    P = torch.randn(E, W, generator=g)
    dd = torch.randn(E, 1, generator=g)
    dd[::3] = 0.0
    return P.to(device), dd.to(device)


def _kill_rows(seq, P):
    """Overwrite every 7th row of P with a vector x such that W1 x + b1 < 0 in every unit."""
    W1, b1 = seq[0].weight.detach().double(), seq[0].bias.detach().double()
    x = torch.linalg.lstsq(W1, (-(b1.abs() + 1.0)).unsqueeze(1)).solution.squeeze(1)  # W1 x = -(|b1| + 1)
    P = P.clone()
    P[::7] = x.to(P.dtype)
    return P


def _run(fn, seq, P, dd, keep=False):
    P = P.clone().requires_grad_(True)
    if not keep:
        for prm in seq.parameters():
            prm.grad = None
    y = fn(seq, P)
    y.backward(dd)
    return [y.detach(), P.grad] + [prm.grad.clone() for prm in seq.parameters()]


def _aten(seq, P):
    return seq(P)


def _within(ours, aten, ref, what):
    dev = (aten.double() - ref).abs().max().item()
    err = (ours.double() - ref).abs().max().item()
    scale = ref.abs().max().item() if ref.numel() else 0.0
    print(f"{what}: err {err:.3e}  aten fp32 {dev:.3e}  scale {scale:.3e}")
    assert err <= 10 * dev + 1e-6 * scale + 1e-12, f"{what}: err {err:.3e} vs aten fp32 {dev:.3e}"


# ------------------------------------------------------------------------------------------ 1. parity
def _parity(device, E):
    seq = _head(E, device)
    P, dd = _inputs(E, device)
    P = _kill_rows(seq, P)
    assert depth_head.fusable(seq, P)
    ours = _run(depth_head.apply, seq, P, dd)
    aten = _run(_aten, seq, P, dd)
    seq64 = _head(E, device, torch.float64)
    seq64.load_state_dict({k: v.double() for k, v in seq.state_dict().items()})
    ref = _run(_aten, seq64, P.double(), dd.double())
    y1 = seq[0](P[::7])
    assert bool((y1 < 0).all()), "the killed rows must have an all-zero first ReLU mask"
    assert bool((ours[1][::7] == 0).all()), "dP of a row with an all-zero mask"
    for o, a, r, name in zip(ours, aten, ref, NAMES):
        assert o.shape == r.shape and o.dtype == torch.float32, name
        _within(o, a, r, f"E={E} {name}")
    again = _run(depth_head.apply, seq, P, dd)
    for o, a, name in zip(ours, again, NAMES):
        assert torch.equal(o, a), f"E={E} {name} not deterministic"
    return seq, P, dd, ours


def test_parity(device):
    for E in SIZES:
        _parity(device, E)

    # E = 0: shapes, zero parameter gradients, no launch
    seq = _head(0, device)
    P0 = torch.zeros(0, W, device=device, requires_grad=True)
    y = depth_head.apply(seq, P0)
    assert y.shape == (0, 1)
    y.sum().backward()
    assert P0.grad.shape == (0, W)
    assert all(prm.grad.shape == prm.shape and float(prm.grad.abs().sum()) == 0.0 for prm in seq.parameters())

    # accumulation into existing .grad tensors == the sum of two separate backward passes
    seq = _head(5, device)
    Pa, da = _inputs(1000, device, seed=11)
    Pb, db = _inputs(777, device, seed=12)
    ga = _run(depth_head.apply, seq, Pa, da)[2:]
    gb = _run(depth_head.apply, seq, Pb, db)[2:]
    for prm in seq.parameters():
        prm.grad = None
    _run(depth_head.apply, seq, Pa, da, keep=True)
    acc = _run(depth_head.apply, seq, Pb, db, keep=True)[2:]
    for a, b, s, name in zip(ga, gb, acc, NAMES[2:]):
        assert torch.equal(a + b, s), f"{name}: accumulated gradient is not the sum of the two passes"


# ------------------------------------------------------------------------------------------ 2. guards
GUARD, PART_GUARD = 16, 2
SENTINEL = 0x7FA5A5A5  # a NaN bit pattern no computation produces


def _bits(t):
    return t.view(torch.int32)


def _sentinel(shape, device):
    return torch.full(shape, SENTINEL, dtype=torch.int32, device=device).view(torch.float32)


def _weights(seq):
    return [seq[0].weight, seq[0].bias, seq[2].weight, seq[2].bias, seq[4].weight, seq[4].bias]


def _call(w, P, dd, d, dP, part_a, part_b):
    _binding.fwd(P, *w, d)
    _binding.bwd(P, *w[:5], dd, dP, part_a, part_b)


def _run_plain(w, P, dd, E, device):
    res = {"d": torch.empty(E, device=device), "dP": torch.empty(E, W, device=device),
           "part_a": torch.empty(_binding.part_shape(E, 0), device=device),
           "part_b": torch.empty(_binding.part_shape(E, 1), device=device)}
    _call(w, P, dd, **res)
    return res


def _run_guarded(w, P, dd, E, device, part_fill):
    """P and dd the first E rows of buffers with NaN tails; d, dP pre-filled with the sentinel and
    followed by guard rows; the partials pre-filled with part_fill and followed by guard rows."""
    Pbig = torch.full((E + GUARD, W), float("nan"), device=device)
    Pbig[:E] = P
    ddbig = torch.full((E + GUARD,), float("nan"), device=device)
    ddbig[:E] = dd.reshape(-1)
    bufs = {"d": _sentinel((E + GUARD,), device), "dP": _sentinel((E + GUARD, W), device)}
    for k, which in (("part_a", 0), ("part_b", 1)):
        rows, cols = _binding.part_shape(E, which)
        bufs[k] = torch.full((rows + PART_GUARD, cols), part_fill, device=device)
    rows = {"d": E, "dP": E, "part_a": bufs["part_a"].shape[0] - PART_GUARD,
            "part_b": bufs["part_b"].shape[0] - PART_GUARD}
    t = {k: b[:rows[k]] for k, b in bufs.items()}
    before = {k: _bits(b).clone() for k, b in bufs.items()}
    _call(w, Pbig[:E], ddbig[:E], **t)
    res = {}
    for k, b in bufs.items():
        n = rows[k]
        assert torch.equal(_bits(b)[n:], before[k][n:]), f"{k} written past row {n}"
        if k in ("d", "dP"):
            assert not bool((_bits(t[k]) == SENTINEL).any()), f"{k} has unwritten elements"
        assert bool(torch.isfinite(t[k]).all()), f"{k} not finite (a poisoned tail was read, or a partial left)"
        res[k] = t[k].clone()
    return res


@pytest.mark.parametrize("E", [1, 17, 1000])
def test_guards(device, E):
    seq = _head(100 + E, device)
    w = _weights(seq)
    P, dd = _inputs(E, device, seed=500 + E)
    with torch.no_grad():
        plain = _run_plain(w, P, dd.reshape(-1), E, device)
        first = None
        for fill in (float("nan"), 1e30, float("nan")):
            res = _run_guarded(w, P, dd, E, device, fill)
            first = first or res
            for k, v in res.items():
                assert torch.equal(_bits(v), _bits(first[k])), f"{k} depends on what its buffer held"
        for k, v in first.items():
            assert torch.equal(_bits(v), _bits(plain[k])), f"{k} differs from the exact-size run"
        # the partial rows sum to the autograd Function's gradients
        ta, tb = _native.colsum(first["part_a"]), _native.colsum(first["part_b"])
    grads = _run(depth_head.apply, seq, P, dd)
    assert torch.equal(grads[0].reshape(-1), first["d"]) and torch.equal(grads[1], first["dP"])
    assert torch.equal(grads[2].reshape(-1), ta[:W * W]) and torch.equal(grads[3], ta[W * W:])
    assert torch.equal(grads[4].reshape(-1), tb[:W * W]) and torch.equal(grads[5], tb[W * W:W * W + W])
    assert torch.equal(grads[6].reshape(-1), tb[W * W + W:W * W + 2 * W]) and torch.equal(grads[7], tb[W * W + 2 * W:])


def test_entry_point_contracts(device):
    """E = 0 is GASFM_OK without a launch (null pointers allowed); a null or misaligned pointer with
    E > 0 is GASFM_ERR_INVALID."""
    L = _binding.lib()
    seq = _head(3, device)
    w = [t.data_ptr() for t in _weights(seq)]
    E = 20
    buf = torch.zeros(E + 1, W, device=device)
    d, dd, dP = torch.zeros(E, device=device), torch.zeros(E, device=device), torch.zeros(E + 1, W, device=device)
    pa = torch.zeros(_binding.part_shape(E, 0), device=device)
    pb = torch.zeros(_binding.part_shape(E, 1), device=device)
    st = _native._stream(buf)
    assert L.gasfm_depth_head_fwd(None, 0, *[None] * 6, None, st) == _native.GASFM_OK
    assert L.gasfm_depth_head_bwd(None, 0, *[None] * 5, None, None, None, None, st) == _native.GASFM_OK
    assert L.gasfm_depth_head_fwd(buf.data_ptr(), -1, *w, d.data_ptr(), st) == _native.GASFM_ERR_INVALID
    assert L.gasfm_depth_head_fwd(buf.data_ptr(), E, *w, d.data_ptr(), st) == _native.GASFM_OK
    assert L.gasfm_depth_head_fwd(None, E, *w, d.data_ptr(), st) == _native.GASFM_ERR_INVALID
    assert L.gasfm_depth_head_fwd(buf.data_ptr(), E, *w, None, st) == _native.GASFM_ERR_INVALID
    assert L.gasfm_depth_head_fwd(buf.data_ptr() + 4, E, *w, d.data_ptr(), st) == _native.GASFM_ERR_INVALID
    assert b"gasfm_depth_head_fwd" in L.gasfm_last_error()
    args = lambda P=buf.data_ptr(), g=dP.data_ptr(), a=pa.data_ptr(): (  # noqa: E731
        P, E, *w[:5], dd.data_ptr(), g, a, pb.data_ptr(), st)
    assert L.gasfm_depth_head_bwd(*args()) == _native.GASFM_OK
    assert L.gasfm_depth_head_bwd(*args(P=None)) == _native.GASFM_ERR_INVALID
    assert L.gasfm_depth_head_bwd(*args(a=None)) == _native.GASFM_ERR_INVALID
    assert L.gasfm_depth_head_bwd(*args(g=dP.data_ptr() + 8)) == _native.GASFM_ERR_INVALID
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ 3. memory, capture
def _peak_new_bytes(fn, seq, P, dd):
    """Peak of newly allocated bytes over one forward + backward with P, dd's source and the weights resident."""
    for prm in seq.parameters():
        prm.grad = None
    Pg = P.detach().requires_grad_(True)  # shares P's storage
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    y = fn(seq, Pg)
    y.backward(dd)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del y, Pg
    return peak


def test_memory_and_capture(device):
    E = 40_013
    seq = _head(9, device)
    P, dd = _inputs(E, device)
    p_bytes = P.numel() * 4
    _run(depth_head.apply, seq, P, dd)  # warm up: the library, occupancy queries, colsum counters
    _run(_aten, seq, P, dd)
    fused = _peak_new_bytes(depth_head.apply, seq, P, dd)
    aten = _peak_new_bytes(_aten, seq, P, dd)
    print(f"peak new bytes over P ({p_bytes}): fused {fused} = {fused / p_bytes:.3f}x, aten {aten} = {aten / p_bytes:.3f}x")
    assert fused < 2 * p_bytes, f"fused head allocates {fused / p_bytes:.2f}x the bytes of P"
    assert aten > 3 * p_bytes, f"aten allocates only {aten / p_bytes:.2f}x the bytes of P: the comparison shows nothing"

    # captured on one stream, replayed: bitwise the eager results
    eager = _run(depth_head.apply, seq, P, dd)
    for prm in seq.parameters():
        prm.grad = None
    Pg = P.clone().requires_grad_(True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):  # warm-up on the capture stream; leaves .grad tensors for the graph to fill
            Pg.grad = None
            for prm in seq.parameters():
                prm.grad = None
            depth_head.apply(seq, Pg).backward(dd)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    Pg.grad = None
    for prm in seq.parameters():
        prm.grad = None
    with torch.cuda.graph(graph):
        y = depth_head.apply(seq, Pg)
        y.backward(dd)
    outs = [y, Pg.grad] + [prm.grad for prm in seq.parameters()]
    for o in outs:
        o.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for o, e, name in zip(outs, eager, NAMES):
        assert torch.equal(o, e), f"{name}: the captured replay differs from the eager run"


def test_other_heads_not_fused(device):
    """Only the fp32 128-128-128-1 no-norm head on contiguous device rows is fused; the rest keeps aten."""
    P = torch.randn(50, W, device=device)
    assert depth_head.fusable(_head(1, device), P)
    assert not depth_head.fusable(_head(1, device), P.double())
    assert not depth_head.fusable(_head(1, device, torch.float64), P)
    assert not depth_head.fusable(_head(1, device), P.cpu()) and not depth_head.fusable(_head(1, "cpu"), P)
    assert not depth_head.fusable(_head(1, device), torch.randn(50, 2 * W, device=device)[:, :W])  # strided rows
    assert not depth_head.fusable(get_linear_layers(3 * [64] + [1], norm=False).to(device), P[:, :64].contiguous())
    assert not depth_head.fusable(get_linear_layers(2 * [W] + [1], norm=False).to(device), P)
    assert not depth_head.fusable(get_linear_layers(4 * [W] + [1], norm=False).to(device), P)
    assert not depth_head.fusable(get_linear_layers(3 * [W] + [1], norm=True).to(device), P)
    assert not depth_head.fusable(get_linear_layers(3 * [W] + [3], norm=False).to(device), P)

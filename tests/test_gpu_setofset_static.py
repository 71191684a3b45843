"""SetOfSetNet through the padded shape-stable union batch (static_batch.StaticBatch) on the MI355X.

  * gasfm_sos_union_tables against the host formulas on hand-made arrays that hit its edges, and
    against ``fill_torch`` on a sampled batch: integer tables bitwise, fp64 tables rtol 1e-15 (each is
    one division of exact integers: a correctly rounded divide gives equality, the margin covers one
    that is not);
  * the fused segment sums over the padded camera plan (every camera through partial slots and one
    combine entry) against an fp64 index_add: |err| <= 1e-5 sum|terms| (/ deg for the mean);
  * the eager padded step against the eager union (``forward_batch`` + summed ESFMLoss): outputs rtol
    1e-4 / atol 1e-5, loss and per-scene reprojection errors rtol 1e-5, gradients at conftest.check_grad's
    bound against the fp64 composite run scene by scene (its fp32 run as ref32); the same after the
    bucket is refilled with another batch (tables rewritten, nothing cached from the first).

Scenes as tests/test_gpu_batch.py: 40-view windowed scenes with 3000 points sampled to 10-18 views;
the shipped dpesfm conf with deterministic weights.
"""
import copy

import numpy as np
import pytest
import torch

import gasfm_amd
from conftest import check_grad
from gasfm_amd import _native, evaluation, static_batch
from gasfm_amd.batch import forward_batch
from gasfm_amd.loss import ESFMLoss
from oracle.weights import deterministic_state_dict
from test_gpu_batch import _grads
from test_gpu_setofset_batch import loss_conf, model_case
from test_gpu_static_batch import _eager, _scenes

pytestmark = pytest.mark.gpu

I32_TABLES = ("ptrc", "ptrp", "ptre")
F64_TABLES = ("Es", "degc", "invc", "wc", "degp", "invp", "wp")
I64_TABLES = ("sop", "soe")


@pytest.fixture(autouse=True)
def s2g_pieces(monkeypatch):
    monkeypatch.setattr(static_batch, "S2G_PIECES", 128)  # the test scenes have ~1-2k valid points


def fresh_net(device):
    conf = loss_conf("shipped")
    net = gasfm_amd.SetOfSetNet(conf)
    net.load_state_dict(deterministic_state_dict(net.state_dict()))
    return net.to(device), ESFMLoss(conf)


# ------------------------------------------------------------------ the tables kernel
def hand_arrays():
    """Five scenes, the middle one without cameras, points and edges; M = 257; the last point of every
    other scene (and more) has no edge; one camera has none.  Host lists and numpy arrays."""
    ms, ns = [60, 70, 0, 64, 63], [300, 200, 0, 150, 127]
    cam, pt, eoff = [], [], [0]
    c0 = p0 = 0
    for s, (m, n) in enumerate(zip(ms, ns)):
        for c in range(m):
            deg = 0 if (s == 3 and c == 5) else 3 + (5 * c + s) % 9
            pts = sorted({(11 * c + 7 * j) % (n - 1) for j in range(deg)})
            cam += [c0 + c] * len(pts)
            pt += [p0 + p for p in pts]
        c0, p0 = c0 + m, p0 + n
        eoff.append(len(cam))
    cam, pt = np.array(cam), np.array(pt)
    M, N = sum(ms), sum(ns)
    return dict(ms=ms, ns=ns, M=M, N=N, E=len(cam), S=len(ms), cam=cam, pt=pt, eoff=np.array(eoff),
                cam_ptr=np.concatenate([[0], np.cumsum(np.bincount(cam, minlength=M))]),
                pt_ptr=np.concatenate([[0], np.cumsum(np.bincount(pt, minlength=N))]),
                soc=np.repeat(np.arange(len(ms)), ms), sop=np.repeat(np.arange(len(ns)), ns))


class _Out:
    pass


def test_union_tables_on_hand_made_arrays(device):
    h = hand_arrays()
    M, N, E, S = h["M"], h["N"], h["E"], h["S"]
    assert M == 257 and N > 256 and N % 256 and E > 256 and E % 256
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=device)
    ins = [i32(h[k]) for k in ("cam_ptr", "pt_ptr", "soc", "sop", "cam", "eoff")]
    size = dict(ptrc=S + 1, ptrp=S + 1, ptre=S + 1, Es=S, degc=M, invc=M, wc=M, degp=N, invp=N, wp=N, sop=N, soe=E)
    G, out, bufs = 3, _Out(), {}
    for names, dtype, sentinel in ((I32_TABLES, torch.int32, -77), (F64_TABLES, torch.float64, -7.5),
                                   (I64_TABLES, torch.int64, -77)):
        for k in names:
            bufs[k] = torch.full((size[k] + 2 * G,), sentinel, dtype=dtype, device=device)  # sentinel rows around
            setattr(out, k, bufs[k][G:G + size[k]])
    _native.sos_union_tables(_native.sos_tables_args(*ins, out), ins[0])
    torch.cuda.synchronize()
    degc, degp = np.bincount(h["cam"], minlength=M).astype(np.float64), np.bincount(h["pt"], minlength=N).astype(
        np.float64)
    assert degc.min() == 0 and degp.min() == 0
    Es = np.maximum(np.diff(h["eoff"]), 1).astype(np.float64)
    assert np.diff(h["eoff"])[2] == 0 and Es[2] == 1.0
    inv = lambda d: np.where(d > 0, 1.0 / np.maximum(d, 1.0), 0.0)
    ref = dict(ptrc=np.concatenate([[0], np.cumsum(h["ms"])]), ptrp=np.concatenate([[0], np.cumsum(h["ns"])]),
               ptre=h["eoff"], Es=Es, degc=degc, invc=inv(degc), wc=degc / Es[h["soc"]], degp=degp, invp=inv(degp),
               wp=degp / Es[h["sop"]], sop=h["sop"], soe=h["soc"][h["cam"]])
    assert ref["ptrc"][2] == ref["ptrc"][3] and ref["ptrc"][-1] == M and ref["ptrp"][-1] == N
    for k, buf in bufs.items():
        got = getattr(out, k).cpu().numpy()
        if k in F64_TABLES:
            np.testing.assert_allclose(got, ref[k], rtol=1e-15, atol=0.0, err_msg=k)
        else:
            assert (got == ref[k]).all(), k
        sentinel = -7.5 if k in F64_TABLES else -77
        assert bool((buf[:G] == sentinel).all()) and bool((buf[G + size[k]:] == sentinel).all()), k
    assert float(out.invp[h["ns"][0] - 1]) == 0.0 and float(out.invc[130 + 5]) == 0.0


def test_union_tables_rejects_bad_arguments(device):
    h = hand_arrays()
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=device)
    ins = [i32(h[k]) for k in ("cam_ptr", "pt_ptr", "soc", "sop", "cam", "eoff")]
    out = _Out()
    for k in I32_TABLES + F64_TABLES + I64_TABLES:
        setattr(out, k, torch.zeros(1, device=device))
    with pytest.raises(ValueError, match="ptrc"):
        _native.sos_tables_args(*ins, out)
    with pytest.raises(ValueError, match="cam_ptr"):
        _native.sos_tables_args(ins[0][:-1], *ins[1:], out)


_FILLED = {}


def filled_batch(device):
    """One sampled batch filled into a bucket by the kernels (with the tables), once.  Every camera of
    a 3000-point scene has more than 256 edges (two or three pieces); the third scene has 900 points,
    so its cameras have one piece each: the one-slot, one-entry combine."""
    if not _FILLED:
        datas = _scenes(device, (12, 15), seed=4) + _scenes(device, (18,), seed=5, n=900)
        st = static_batch.BatchStats(datas)
        assert st.expressible() is None
        sb = static_batch.StaticBatch(static_batch.Caps.for_batch(st), device)
        sb.sos_tables()
        sb.fill(datas, st)
        _FILLED.update(datas=datas, st=st, sb=sb)
    return _FILLED


def test_union_tables_match_fill_torch(device):
    f = filled_batch(device)
    a = f["sb"]
    b = static_batch.StaticBatch(a.caps, device)
    tb = b.sos_tables()
    b.fill_torch(f["datas"], f["st"])
    ta = a.sos_tables()
    for k in I32_TABLES + I64_TABLES + ("soc", "ptr_all_c"):
        assert torch.equal(getattr(ta, k), getattr(tb, k)), k
    for k in F64_TABLES:
        torch.testing.assert_close(getattr(ta, k), getattr(tb, k), rtol=1e-15, atol=0.0, msg=lambda m: f"{k}: {m}")
    mo, no, eo = a.offsets
    assert ta.ptrc.tolist() == mo + [a.caps.M] and ta.ptre.tolist() == eo + [a.caps.E]


# ------------------------------------------------------------------ segment sums over the padded camera plan
@pytest.mark.parametrize("width", [2, 32, 256])
def test_segment_sums_over_the_padded_camera_plan(device, width):
    f = filled_batch(device)
    sb, st = f["sb"], f["st"]
    plan = sb.graph_wrappers["proj2view"].plan
    pieces = sb.comb_c[:, 2]
    assert plan.n_slots == sb.caps.I and plan.n_combine == sb.caps.M and not plan.all_partial
    assert bool((pieces[:st.M] == 1).any())        # a real camera through one partial slot and a one-entry combine
    assert bool((pieces[st.M:] > 1).all())         # every pad camera has several pieces
    g = torch.Generator().manual_seed(width)
    X = torch.randn(sb.caps.E, width, generator=g).to(device)
    Ym = torch.randn(sb.caps.E, width, generator=g).to(device)
    cam = sb.cam32.long()
    deg = torch.bincount(cam, minlength=sb.caps.M).double()
    assert float(deg.min()) >= 1
    for mask in (None, Ym):
        T = X.double() if mask is None else X.double() * (mask > 0)
        z = torch.zeros(sb.caps.M, width, dtype=torch.float64, device=device)
        tot, mag = z.index_add(0, cam, T), z.index_add(0, cam, T.abs())
        for mean in (False, True):
            got = _native.sos_segment_sum(plan, X, mean=mean, mask=mask)
            div = deg[:, None] if mean else 1.0
            err, bound = (got.double() - tot / div).abs(), 1e-5 * mag / div
            print(f"width {width} mask {mask is not None} mean {mean}: max err {float(err.max()):.3e}, "
                  f"bound there {float(bound.flatten()[err.argmax()]):.3e}")
            assert bool((err <= bound).all()), (mean, mask is not None, float((err - bound).max()))
            assert torch.equal(_native.sos_segment_sum(plan, X, mean=mean, mask=mask), got)


# ------------------------------------------------------------------ the padded step
def composite_grads(net, lossf, datas, inputs=None):
    """Parameter gradients of the summed ESFMLoss with the torch-op composite run scene by scene, in
    fp64 and fp32, on a copy of the net (a captured graph holds the addresses of the net's own
    weights).  The loss kernels are fp32: the fp64 run hands them its predictions rounded to fp32."""
    ref = copy.deepcopy(net)
    ref.composite = True
    inputs = datas if inputs is None else inputs
    vals32 = [d.x.values for d in inputs]
    out = []
    try:
        for dtype in (torch.float64, torch.float32):
            ref.to(dtype)
            for p in ref.parameters():
                p.grad = None
            loss = 0
            for din, d, v in zip(inputs, datas, vals32):
                din.x.values = v.to(dtype)
                p = ref(din)
                loss = loss + lossf({k: p[k].float() for k in ("Ps_norm", "pts3D")}, d)
            loss.backward()
            out.append({k: p.grad.detach().double().cpu().numpy() for k, p in ref.named_parameters()})
    finally:
        for din, v in zip(inputs, vals32):
            din.x.values = v
    return out


def check_grads_fp64(net, grads, g64, g32, what):
    for (k, _), g in zip(net.named_parameters(), grads):
        check_grad(g, g64[k], f"{what} {k}", ref32=g32[k])


def union_errors(net, datas, inputs=None):
    with torch.no_grad():
        preds = forward_batch(net, datas if inputs is None else inputs)
    return preds, [float(evaluation.reprojection_error_mean(d, p)) for p, d in zip(preds, datas)]


def check_outputs(sb, pred, pred_ref):
    for i, (a, b) in enumerate(zip(sb.split(pred), pred_ref)):
        for k in ("Ps_norm", "pts3D"):
            np.testing.assert_allclose(a[k].detach().cpu().numpy(), b[k].detach().cpu().numpy(), rtol=1e-4, atol=1e-5,
                                       err_msg=f"scene {i} {k}")
    assert torch.isfinite(pred["Ps_norm"]).all() and torch.isfinite(pred["pts3D"]).all()  # the pad scene too


def padded_eager(net, lossf, sb):
    """net(sb) + batch_loss + backward on the buffers the last fill wrote."""
    net.zero_grad(set_to_none=True)
    pred = net(sb)
    loss = static_batch.batch_loss(pred, sb, lossf)
    tot = static_batch.batch_repro_errors(pred, sb)
    loss.backward()
    return pred, loss.detach(), tot, _grads(net)


def test_padded_step_matches_the_eager_union(device):
    case = model_case(device, "shipped")   # the union, and the fp64 / fp32 composite per-scene loops, computed once
    net, datas = case["net"], case["datas"]
    lossf = ESFMLoss(loss_conf("shipped"))
    o_ref, _, loss_ref = case["u1"]
    _, err_ref = union_errors(net, datas)
    st = static_batch.BatchStats(datas)
    assert st.expressible() is None
    sb = static_batch.StaticBatch(static_batch.Caps.for_batch(st), device)
    sb.fill(datas, st)
    with _native.dispatch_record() as rec:
        pred, loss, tot, g = padded_eager(net, lossf, sb)
    assert rec.counts["sos_edge_fwd"] == 3   # the fused path was taken: one edge kernel per layer
    check_outputs(sb, pred, o_ref)
    assert abs(float(loss) - loss_ref) <= 1e-5 * abs(loss_ref)
    np.testing.assert_allclose([a / b for a, b in tot.tolist()[:st.B]], err_ref, rtol=1e-5)
    g64 = {k: v.cpu().numpy() for k, v in case["c64"][1].items()}
    g32 = {k: v.double().cpu().numpy() for k, v in case["c32"][1].items()}
    check_grads_fp64(net, g, g64, g32, "padded")
    for p in net.parameters():
        p.grad = None



def test_refilled_bucket_gives_the_second_batch(device):
    """One bucket filled with a batch, then with another: the second padded step is the second batch's
    (a table or degree cached from the first fill would show at O(1))."""
    net, lossf = fresh_net(device)
    batches = [_scenes(device, (14, 16, 18), seed=0), _scenes(device, (10, 12, 13), seed=1)]
    sts = [static_batch.BatchStats(b) for b in batches]
    caps = static_batch.Caps.for_batch(sts[0])
    assert caps.pad(sts[1]) is not None
    sb = static_batch.StaticBatch(caps, device)
    for k, (datas, st) in enumerate(zip(batches, sts)):
        g64, g32 = composite_grads(net, lossf, datas)
        sb.fill(datas, st)
        pred, loss, tot, g = padded_eager(net, lossf, sb)
        pred_ref, loss_ref, _, err_ref = _eager(net, lossf, datas)
        check_outputs(sb, pred, pred_ref)
        assert abs(float(loss) - loss_ref) <= 1e-5 * abs(loss_ref), k
        np.testing.assert_allclose([a / b for a, b in tot.tolist()[:st.B]], err_ref, rtol=1e-5)
        check_grads_fp64(net, g, g64, g32, f"batch {k}")

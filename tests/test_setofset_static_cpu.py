"""SetOfSetNet over the padded shape-stable union batch (static_batch.StaticBatch), on the CPU in fp64.

The set-of-set layers read each scene's row ranges, the scene of every row, max(E_s, 1) and
deg / E_s from tables the bucket owns and every fill rewrites (StaticBatch.sos_tables; fill_torch is
the CPU path and the HIP kernel's oracle).  Checked here: the tables against the batch's host lists,
the composite forward and backward through the padded batch against the net run scene by scene, a
refill of the same bucket with another batch.

Bars: outputs rtol 1e-10 elementwise; parameter gradients of a summed linear functional of the real
scenes' outputs normwise 1e-9, over the whole gradient and for every tensor that carries more than
1e-6 of its norm (the biases in front of a centring have a gradient that is zero in exact
arithmetic: ~1e-18 of rounding on both sides, which no relative bar can hold).
"""
import numpy as np
import pytest
import torch

import gasfm_amd
from gasfm_amd import static_batch, synthetic
from gasfm_amd.conf import dpesfm_conf
from gasfm_amd.scene import SceneData
from oracle.weights import deterministic_state_dict


@pytest.fixture(autouse=True)
def small_pieces(monkeypatch):
    monkeypatch.setattr(static_batch, "S2G_PIECES", 16)


def small_scenes(seed=0, views=(8, 9, 11), n=260):
    out = []
    for i, m in enumerate(views):
        sc = synthetic.windowed_scene(m, n + 20 * i, mean_extra=4, seed=50 + 10 * seed + i)
        out.append(SceneData(torch.from_numpy(sc.dense_M()), torch.from_numpy(sc.Ns()), torch.from_numpy(sc.Ps_gt()),
                             f"s{seed}{i}"))
    return out


def small_net():
    net = gasfm_amd.SetOfSetNet(dpesfm_conf(num_features=32))
    net.load_state_dict(deterministic_state_dict(net.state_dict()))
    net.composite = True
    return net.double()


def bucket_for(*batches):
    """One bucket every given batch fits (the sizes of the largest, by edges)."""
    sts = [static_batch.BatchStats(b) for b in batches]
    assert all(st.expressible() is None for st in sts)
    caps = static_batch.Caps.for_batch(max(sts, key=lambda st: st.E))
    assert all(caps.pad(st) is not None for st in sts)
    return static_batch.StaticBatch(caps, torch.device("cpu")), sts


def check_tables(sb, st):
    t, c = sb.sos_tables(), sb.caps
    mp, npd, ep, _ = c.pad(st)
    mo, no, eo = sb.offsets
    assert t.B == c.S == st.B + 1 and t.E == c.E and t.ptr_all_c.tolist() == [0, c.M]
    assert t.ptrc.tolist() == mo + [c.M] and t.ptrp.tolist() == no + [c.N] and t.ptre.tolist() == eo + [c.E]
    assert all(p.dtype == torch.int32 for p in (t.ptrc, t.ptrp, t.ptre, t.ptr_all_c))
    cam, pt = sb.cam32.long(), sb.pt32.long()
    soc = torch.from_numpy(np.repeat(np.arange(c.S), st.ms + [mp]))
    assert torch.equal(t.soc, soc) and torch.equal(t.soe, soc[cam]) and torch.equal(t.sop[pt], t.soe)
    assert t.sop.dtype == t.soe.dtype == torch.int64
    Es = torch.tensor(st.Es + [ep], dtype=torch.float64)
    assert torch.equal(t.Es, Es)
    degc = torch.bincount(cam, minlength=c.M).double()
    degp = torch.bincount(pt, minlength=c.N).double()
    assert torch.equal(t.degc, degc) and torch.equal(t.degp, degp)
    assert degc.min() >= 1 and degp.min() >= 1
    assert torch.equal(t.invc, 1.0 / degc) and torch.equal(t.invp, 1.0 / degp)
    assert torch.equal(t.wc, degc / Es[t.soc]) and torch.equal(t.wp, degp / Es[t.sop])


def test_tables_against_the_host_lists():
    datas = small_scenes()
    sb, (st,) = bucket_for(datas)
    sb.sos_tables()
    sb.fill_torch(datas, st)
    check_tables(sb, st)


def test_tables_made_after_a_fill_hold_that_fill():
    datas = small_scenes()
    sb, (st,) = bucket_for(datas)
    sb.fill(datas, st)
    assert "_scene_tables" not in sb._plans   # a GraphAttnSfMNet bucket never allocates them
    check_tables(sb, st)


def coefficients(datas, seed=3):
    g = torch.Generator().manual_seed(seed)
    return [{"Ps_norm": torch.randn(d.x.shape[0], 3, 4, generator=g, dtype=torch.float64),
             "pts3D": torch.randn(4, d.x.shape[1], generator=g, dtype=torch.float64)} for d in datas]


def run(net, forward, coefs):
    for p in net.parameters():
        p.grad = None
    preds = forward()
    sum((p[k] * c[k]).sum() for p, c in zip(preds, coefs) for k in c).backward()
    return ([{k: p[k].detach().clone() for k in c} for p, c in zip(preds, coefs)],
            {k: p.grad.detach().clone() for k, p in net.named_parameters()})


def padded_against_the_loop(net, sb, st, datas):
    """Fill the bucket with the batch and compare the padded run with the net run scene by scene."""
    for d in datas:
        d.x.values = d.x.values.double()
    coefs = coefficients(datas)
    o_ref, g_ref = run(net, lambda: [net(d) for d in datas], coefs)
    sb.fill(datas, st)
    sb.x.values = sb.values.double()   # the fp64 net's input: the fp32 static buffer widened
    whole = {}

    def padded():
        whole.update(net(sb))
        return sb.split(whole)

    o, g = run(net, padded, coefs)
    assert torch.isfinite(whole["Ps_norm"]).all() and torch.isfinite(whole["pts3D"]).all()   # the pad scene too
    assert whole["Ps_norm"].shape[0] == sb.caps.M and whole["pts3D"].shape[1] == sb.caps.N
    for i, (a, b) in enumerate(zip(o, o_ref)):
        for k in b:
            torch.testing.assert_close(a[k], b[k], rtol=1e-10, atol=0.0, msg=lambda m: f"scene {i} {k}: {m}")
    assert set(g) == set(g_ref)
    tot = float(torch.sqrt(sum(v.norm() ** 2 for v in g_ref.values())))
    err = float(torch.sqrt(sum((g[k] - g_ref[k]).norm() ** 2 for k in g_ref)))
    assert err <= 1e-9 * tot, (err, tot)
    for k, r in g_ref.items():
        if float(r.norm()) > 1e-6 * tot:
            assert float((g[k] - r).norm()) <= 1e-9 * float(r.norm()), k
    return o


def test_padded_batch_matches_the_per_scene_loop_fp64():
    datas = small_scenes()
    sb, (st,) = bucket_for(datas)
    padded_against_the_loop(small_net(), sb, st, datas)


def test_refilled_bucket_gives_the_second_batch():
    first, second = small_scenes(seed=0), small_scenes(seed=1, views=(10, 8, 9), n=240)
    sb, (st1, st2) = bucket_for(first, second)
    net = small_net()
    o1 = padded_against_the_loop(net, sb, st1, first)
    check_tables(sb, st1)
    o2 = padded_against_the_loop(net, sb, st2, second)
    check_tables(sb, st2)
    assert o1[0]["Ps_norm"].shape != o2[0]["Ps_norm"].shape or not torch.equal(o1[0]["Ps_norm"], o2[0]["Ps_norm"])


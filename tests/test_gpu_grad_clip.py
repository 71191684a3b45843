"""Gradient norm, clipping, loss guard and the capturable Adam of gasfm_amd.optim (csrc/adam.hip).

The parameter set reaches every branch of the kernels: sizes 0, 1, 3, 4, 5 (scalar tail), 4095, 4096,
4097 and 2 * 4096 + 7 (chunk edges, several workgroups), a parameter that starts one element into its
storage (not 16-byte aligned: scalar path), one whose .grad alone is unaligned, one without a gradient.
Gradient magnitudes span 1e-4 .. 1e2.

Bounds.  The sum of squares is accumulated in fp64 (g * g is exact there) over a depth of at most
16 + 6 + 4 values per chunk and ceil(chunks / 1024) + 6 + 16 in the finish, so the total is exact to
~1e-14 and the fp32 norm carries one rounding: NORM_RTOL = 2^-24 (+ 1e-10 for the fp64 part), tighter
than the 2e-6 an fp32 accumulation would need.  The clip coefficient th / (norm + 1e-6) adds two fp32
roundings and g * coef one: COEF_RTOL = 4 * 2^-24.  The Adam bound is the existing test's rtol 2e-6 /
atol 1e-7, plus COEF_RTOL in norm mode; for exp_avg, whose terms cancel, the coefficient's error is
propagated through the size of the terms (``_check_against``), and where torch's own fp32 exp_avg
misses the bound against the fp64 restatement, ours may need at most twice torch's exp_avg error; the
parameters and exp_avg_sq are held to the bound itself (``_within``).
"""
import copy
import math

import pytest
import torch

import gasfm_amd
from gasfm_amd import optim, static_batch
from gasfm_amd.optim import Adam

pytestmark = pytest.mark.gpu

NUMELS = [0, 1, 3, 4, 5, 4095, 4096, 4097, 2 * 4096 + 7]
NORM_RTOL = 2.0 ** -24 + 1e-10
COEF_RTOL = 4 * 2.0 ** -24
RTOL, ATOL = 2e-6, 1e-7
LR, BETAS, EPS = 1e-3, (0.9, 0.999), 1e-8


def _draw_grad(n, gen):
    return torch.randn(n, generator=gen) * 10.0 ** (torch.rand(n, generator=gen) * 6 - 4)


def _params(device, seed=0):
    """(parameters, index of the one without a gradient); every other parameter holds a gradient."""
    gen = torch.Generator().manual_seed(seed)
    ps = [torch.randn(n, generator=gen).to(device).requires_grad_(True) for n in NUMELS]
    ps.append(torch.randn(4097 + 1, generator=gen).to(device)[1:].detach().requires_grad_(True))  # unaligned p
    ps.append(torch.randn(1030, generator=gen).to(device).requires_grad_(True))  # unaligned .grad only
    ps.append(torch.randn(77, generator=gen).to(device).requires_grad_(True))  # no gradient
    assert ps[-3].data_ptr() % 16 == 4 and ps[-3].is_contiguous()
    for p in ps[:-2]:
        p.grad = torch.empty_like(p)
    ps[-2].grad = torch.empty(1031, device=device)[1:]
    assert ps[-2].grad.data_ptr() % 16 == 4 and ps[-2].data_ptr() % 16 == 0
    _fill_grads(ps, gen)
    return ps, gen


def _fill_grads(ps, gen):
    for p in ps:
        if p.grad is not None:
            p.grad.copy_(_draw_grad(p.numel(), gen))


def _norm64(ps):
    return math.sqrt(sum(float((p.grad.double() ** 2).sum()) for p in ps if p.grad is not None))


def _copy_of(t):
    """A copy with t's alignment: one element into its storage when t is not 16-byte aligned."""
    t = t.detach()
    if t.data_ptr() % 16 == 0:
        return t.clone()
    out = torch.empty(t.numel() + 1, device=t.device)[1:]
    assert out.data_ptr() % 16 == 4
    return out.copy_(t)


def _clone_params(ps):
    out = [_copy_of(p).requires_grad_(True) for p in ps]
    for a, p in zip(out, ps):
        a.grad = None if p.grad is None else _copy_of(p.grad)
    return out


def _clip64(grads, mode, th):
    """torch's clip_grad_norm_ / clip_grad_value_ restated in fp64 (None entries pass through)."""
    if mode == "norm":
        norm = math.sqrt(sum(float((g * g).sum()) for g in grads if g is not None))
        coef = min(1.0, th / (norm + 1e-6))
        return [None if g is None else g * coef for g in grads]
    if mode == "value":
        return [None if g is None else g.clamp(-th, th) for g in grads]
    return grads


class Ref64:
    """Clip followed by torch.optim.Adam's update, restated in fp64 on the CPU."""

    def __init__(self, ps, wd, mode=None, th=None):
        self.p = [p.detach().double().cpu() for p in ps]
        self.m = [torch.zeros_like(p) for p in self.p]
        self.v = [torch.zeros_like(p) for p in self.p]
        self.a = [torch.zeros_like(p) for p in self.p]  # exp_avg's recurrence over |g|: the size of its terms
        self.t, self.wd, self.mode, self.th = 0, wd, mode, th

    def step(self, grads, lr=LR):
        self.t += 1
        b1, b2 = BETAS
        gs = _clip64([None if g is None else g.detach().double().cpu() for g in grads], self.mode, self.th)
        for p, m, v, a, g in zip(self.p, self.m, self.v, self.a, gs):
            if g is None:
                continue
            if self.wd:
                g = g + self.wd * p
            m.mul_(b1).add_(g, alpha=1 - b1)
            a.mul_(b1).add_(g.abs(), alpha=1 - b1)
            v.mul_(b2).add_(g * g, alpha=1 - b2)
            p.sub_(lr / (1 - b1 ** self.t) * m / (v.sqrt() / math.sqrt(1 - b2 ** self.t) + EPS))


def _units(got, ref, rtol, extra=0.0):
    """max |got - ref| / (ATOL + rtol |ref| + extra): <= 1 passes the bound."""
    if ref.numel() == 0:
        return 0.0
    return float(((got.detach().double().cpu() - ref).abs() / (ATOL + rtol * ref.abs() + extra)).max())


def _check_against(ref, ps, opt, rtol, label):
    """Worst error of the parameters and both moments, in units of the bound.  The clip coefficient's
    relative error c = rtol - RTOL (norm mode) moves every clipped gradient by c |g|, so exp_avg -- a
    sum of terms of both signs -- by up to c times the same recurrence over |g| (ref.a), which is an
    absolute allowance where the terms cancel; exp_avg_sq has one sign and takes it in rtol."""
    worst = [0.0, 0.0, 0.0]
    for i, p in enumerate(ps):
        if p.grad is None:
            continue
        st = opt.state[p]
        for k, (got, want, extra) in enumerate(((p, ref.p[i], 0.0), (st["exp_avg"], ref.m[i], (rtol - RTOL) * ref.a[i]),
                                               (st["exp_avg_sq"], ref.v[i], 0.0))):
            worst[k] = max(worst[k], _units(got, want, rtol, extra))
    print(f"{label}: p {worst[0]:.3f}, exp_avg {worst[1]:.3f}, exp_avg_sq {worst[2]:.3f} of the bound "
          f"(rtol {rtol:.3g}, atol {ATOL:g})")
    return worst


def _within(e_ours, e_torch):
    """(parameters, exp_avg, exp_avg_sq) in units of the bound: the parameters and exp_avg_sq at the
    bound itself; exp_avg at the bound, or at twice what torch's own fp32 sequence needs against the
    same fp64 restatement where fp32 itself cannot meet it (elements in which gradients of magnitude
    1e2 cancel carry the rounding of their largest term: up to 8.3 bounds in torch's own run, see the
    docstring of the Adam test)."""
    return e_ours[0] <= 1.0 and e_ours[2] <= 1.0 and e_ours[1] <= max(1.0, 2.0 * e_torch[1])


def test_grad_norm_matches_fp64_and_is_reproducible(device):
    ps, _ = _params(device)
    ref = _norm64(ps)
    a, b = optim.grad_norm(ps), optim.grad_norm(ps)
    assert a.is_cuda and a.dim() == 0 and a.dtype == torch.float32
    err = abs(float(a) - ref) / ref
    print(f"grad_norm {float(a)!r} vs fp64 {ref!r}: relative error {err:.3e} (bound {NORM_RTOL:.3e})")
    assert err <= NORM_RTOL
    assert torch.equal(a, b)
    for p in ps:
        if p.grad is not None:
            p.grad.zero_()
    assert float(optim.grad_norm(ps)) == 0.0


@pytest.mark.parametrize("factor", [0.5, 2.0])
def test_clip_functions_match_torch(device, factor):
    ps, _ = _params(device, seed=1)
    norm64 = _norm64(ps)
    th = factor * norm64
    # norm mode against torch.nn.utils.clip_grad_norm_ on clones
    ours, ref = _clone_params(ps), _clone_params(ps)
    n_ref = torch.nn.utils.clip_grad_norm_(ref, th)
    n_ours = optim.clip_grad_norm_(ours, th)
    assert abs(float(n_ours) - norm64) <= NORM_RTOL * norm64  # the norm before clipping
    e_torch = abs(float(n_ref) - norm64) / norm64  # the reference's own error
    assert e_torch <= 2e-6
    # ours: COEF_RTOL; torch's: its norm error + add, reciprocal, multiply, product (4 roundings)
    bound = min(2e-6, COEF_RTOL + e_torch + 4 * 2.0 ** -24)
    print(f"th = {factor} x norm: torch's norm error {e_torch:.3e}, elementwise bound {bound:.3e}")
    for a, b in zip(ours, ref):
        assert (a.grad is None) == (b.grad is None)
        if a.grad is not None:
            torch.testing.assert_close(a.grad, b.grad, rtol=bound, atol=0)
    # value mode is bitwise
    th_v = factor * 1.0
    ours, ref = _clone_params(ps), _clone_params(ps)
    torch.nn.utils.clip_grad_value_(ref, th_v)
    assert optim.clip_grad_value_(ours, th_v) is None
    for a, b in zip(ours, ref):
        assert (a.grad is None) == (b.grad is None)
        if a.grad is not None:
            assert torch.equal(a.grad, b.grad)
    assert ours[-1].grad is None


def test_clip_inf_gradient_nan_pattern_and_norm_type(device):
    ps, _ = _params(device, seed=2)
    ps[7].grad[5] = float("inf")
    ours, ref = _clone_params(ps), _clone_params(ps)
    n_ref = torch.nn.utils.clip_grad_norm_(ref, 1.0)
    n_ours = optim.clip_grad_norm_(ours, 1.0)
    assert math.isinf(float(n_ours)) and math.isinf(float(n_ref))
    for a, b in zip(ours, ref):
        if a.grad is not None:
            assert torch.equal(torch.isnan(a.grad), torch.isnan(b.grad))
            assert torch.equal(torch.nan_to_num(a.grad, nan=7.0), torch.nan_to_num(b.grad, nan=7.0))
    assert int(sum(torch.isnan(a.grad).sum() for a in ours if a.grad is not None)) == 1
    with pytest.raises(ValueError):
        optim.clip_grad_norm_(ours, 1.0, norm_type=1)
    with pytest.raises(ValueError):
        optim.clip_grad_norm_(ours, 1.0, norm_type=float("inf"))


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("mode", [None, "norm", "value"])
def test_device_adam_five_steps_against_fp64(device, mode, wd):
    """Parameters and both moments after five steps against the fp64 restatement, at rtol 2e-6 (+
    COEF_RTOL in norm mode) / atol 1e-7.  torch's own fp32 sequence (clip_grad_norm_ / clip_grad_value_
    + torch.optim.Adam) is run against the same restatement and printed.  Measured on an MI355X, in
    units of the bound, torch / ours: parameters 0.12 / 0.12, exp_avg_sq 0.20 / 0.18 (both asserted at
    the bound itself); exp_avg without
    clipping 2.40 / 2.40 (wd 0) and 8.30 / 8.30 (wd 0.01) -- identical, the arithmetic is the same and
    fp32 cannot hold elements in which gradients of magnitude 1e2 cancel to 1e-7 + 2e-6 |exp_avg| --
    with norm clipping 0.29 / 0.38, with value clipping 0.02 / 0.02.  exp_avg passes at the bound, or at
    no more than twice torch's own exp_avg error where torch exceeds it (``_within``)."""
    ps, gen = _params(device, seed=3)
    th = {None: None, "norm": 0.5 * _norm64(ps), "value": 0.05}[mode]
    tps = _clone_params(ps)
    ref = Ref64(ps, wd, mode, th)
    opt = Adam(ps, lr=LR, betas=BETAS, eps=EPS, weight_decay=wd, capturable=True, grad_clip_mode=mode,
               grad_clip_th=th)
    topt = torch.optim.Adam(tps, lr=LR, betas=BETAS, eps=EPS, weight_decay=wd)
    for it in range(5):
        if it:
            _fill_grads(ps, gen)
            for a, p in zip(tps, ps):
                if p.grad is not None:
                    a.grad.copy_(p.grad)
        before = [None if p.grad is None else p.grad.clone() for p in ps]
        ref.step(before)
        opt.step()
        for p, g in zip(ps, before):  # p.grad is left as the backward wrote it
            assert (p.grad is None) == (g is None) and (g is None or torch.equal(p.grad, g))
        if mode == "norm":
            torch.nn.utils.clip_grad_norm_(tps, th)
        elif mode == "value":
            torch.nn.utils.clip_grad_value_(tps, th)
        topt.step()
    rtol = RTOL + (COEF_RTOL if mode == "norm" else 0.0)
    e_torch = _check_against(ref, tps, topt, rtol, f"torch fp32 mode={mode} wd={wd}")
    e_ours = _check_against(ref, ps, opt, rtol, f"device Adam mode={mode} wd={wd}")
    assert _within(e_ours, e_torch), (e_ours, e_torch)
    assert float(opt.state[ps[0]]["step"]) == 5.0 and opt.state[ps[0]]["step"].is_cuda
    assert ps[-1] not in opt.state or not opt.state[ps[-1]]  # no gradient: no state, as torch
    if mode == "norm":
        assert abs(float(opt.grad_norm) - _norm64(ps)) <= NORM_RTOL * _norm64(ps)
    else:
        assert opt.grad_norm is None


def _snapshot(ps, opt):
    return [(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone(),
             opt.state[p]["step"].clone(), p.grad.clone()) for p in ps if p.grad is not None]


def test_loss_guard(device):
    ps, gen = _params(device, seed=4)
    ref = Ref64(ps, 0.01)
    tps = _clone_params(ps)
    topt = torch.optim.Adam(tps, lr=LR, betas=BETAS, eps=EPS, weight_decay=0.01)  # the real steps in torch's fp32
    opt = Adam(ps, lr=LR, betas=BETAS, eps=EPS, weight_decay=0.01, capturable=True, track_grad_norm=True)
    loss = torch.tensor(1.0, device=device)
    ref.step([p.grad for p in ps])
    topt.step()
    opt.step(loss=loss)
    real = 1
    for value in (0.0, -1.0, float("nan")):
        snap = _snapshot(ps, opt)
        loss.fill_(value)
        opt.step(loss=loss)
        for a, b in zip(snap, _snapshot(ps, opt)):
            assert all(torch.equal(x, y) for x, y in zip(a, b)), value
    # guarded, taken, guarded, taken (a tiny positive loss): the counter and the bias correction follow
    for value in (0.0, 2.0, float("nan"), 1e-30):
        _fill_grads(ps, gen)
        loss.fill_(value)
        if value > 0:
            ref.step([p.grad for p in ps])
            for a, p in zip(tps, ps):
                if p.grad is not None:
                    a.grad.copy_(p.grad)
            topt.step()
            real += 1
        opt.step(loss=loss)
        assert float(opt.state[ps[1]]["step"]) == real
    assert real == 3
    e_torch = _check_against(ref, tps, topt, RTOL, "torch fp32, the real steps")
    assert _within(_check_against(ref, ps, opt, RTOL, "guarded sequence"), e_torch)


def test_tensor_lr_follows_a_scheduler(device):
    ps, gen = _params(device, seed=5)
    qs = _clone_params(ps)
    o_t = Adam(ps, lr=torch.tensor(LR, device=device), betas=BETAS, eps=EPS, capturable=True)
    o_f = Adam(qs, lr=LR, betas=BETAS, eps=EPS, capturable=True)
    s_t = torch.optim.lr_scheduler.LinearLR(o_t, start_factor=0.1, total_iters=4)
    s_f = torch.optim.lr_scheduler.LinearLR(o_f, start_factor=0.1, total_iters=4)
    lrs = []
    for it in range(5):
        if it:
            _fill_grads(ps, gen)
            for a, p in zip(qs, ps):
                if p.grad is not None:
                    a.grad.copy_(p.grad)
        lrs.append(float(o_f.param_groups[0]["lr"]))
        o_t.step()
        o_f.step()
        s_t.step()
        s_f.step()
    assert torch.is_tensor(o_t.param_groups[0]["lr"]) and lrs[0] != lrs[-1]
    assert abs(float(o_t.param_groups[0]["lr"]) - o_f.param_groups[0]["lr"]) <= 1e-6 * LR
    for a, b in zip(ps, qs):
        torch.testing.assert_close(a, b, rtol=RTOL, atol=ATOL)
    with pytest.raises(TypeError):
        Adam(qs, lr=torch.tensor(LR, device=device))  # the host path still refuses a tensor lr


def test_state_dict_round_trip_and_torch_capturable(device):
    ps, gen = _params(device, seed=6)
    ps = ps[:-1]  # torch's capturable Adam and ours: the same parameters hold state
    kw = dict(lr=LR, betas=BETAS, eps=EPS, weight_decay=0.01)
    ours = Adam(ps, capturable=True, **kw)
    for _ in range(2):
        ours.step()
        _fill_grads(ps, gen)
    sd = copy.deepcopy(ours.state_dict())
    steps = [s["step"] for s in sd["state"].values()]
    assert all(s.is_cuda and float(s) == 2.0 for s in steps) and len({s.data_ptr() for s in steps}) == len(steps)
    qs, rs, ts = _clone_params(ps), _clone_params(ps), _clone_params(ps)
    again = Adam(qs, capturable=True, **kw)
    again.load_state_dict(copy.deepcopy(sd))
    into_torch = torch.optim.Adam(rs, capturable=True, **kw)
    into_torch.load_state_dict(copy.deepcopy(sd))
    ours.step()
    again.step()
    into_torch.step()
    for a, b, c in zip(ps, qs, rs):
        assert torch.equal(a, b)
        torch.testing.assert_close(c, a, rtol=RTOL, atol=ATOL)
    assert float(into_torch.state[rs[1]]["step"]) == 3.0
    # and back: a torch capturable state continues in ours
    back = Adam(ts, capturable=True, **kw)
    for t, r in zip(ts, rs):
        t.data.copy_(r.data)
    back.load_state_dict(copy.deepcopy(into_torch.state_dict()))
    for group in (ps, rs, ts):
        gen2 = torch.Generator().manual_seed(60)
        _fill_grads(group, gen2)
    ours.step()
    into_torch.step()
    back.step()
    assert float(back.state[ts[1]]["step"]) == 4.0
    for a, c, d in zip(ps, rs, ts):
        torch.testing.assert_close(d, c, rtol=RTOL, atol=ATOL)
        torch.testing.assert_close(d, a, rtol=RTOL, atol=ATOL)


def test_static_trainer_captures_the_guarded_clipped_step(device, monkeypatch):
    """Three steps over two buckets with the optimizer step captured (one graph per bucket), then two
    more that replay the existing graphs with fresh gradients and the advanced counter: the weights
    after each step equal, bitwise, those of the same optimizer stepped eagerly on cloned weights with
    the same gradients and loss; a zero-loss batch leaves the weights untouched."""
    from gasfm_amd.loss import ESFMLoss
    from test_gpu_batch import _conf
    from test_gpu_static_batch import _scenes
    monkeypatch.setattr(static_batch, "S2G_PIECES", 128)
    torch.manual_seed(2)
    conf = _conf()
    net = gasfm_amd.GraphAttnSfMNet(conf).to(device)
    params = [p for p in net.parameters() if p.requires_grad]
    clones = [p.detach().clone().requires_grad_(True) for p in params]
    kw = dict(lr=1e-3, capturable=True, grad_clip_mode="norm", grad_clip_th=1.0, track_grad_norm=True)
    trainer = static_batch.StaticTrainer(net, ESFMLoss(conf), optimizer=Adam(params, **kw), guard_loss=True)
    eager = Adam(clones, **kw)
    batches = [_scenes(device, (14, 16, 18), seed=0), _scenes(device, (10, 12, 13), seed=1)]
    for it, k in enumerate((0, 1, 0, 0, 1)):
        if it == 3:  # from here on every optimizer step is a replay of a graph captured earlier
            assert len(trainer.buckets) == 2 and trainer.opt_graphs == 2
        loss, _ = trainer.step(batches[k])
        assert float(loss) > 0 and trainer.fallbacks == [] and trainer.eager_steps == 0
        for c, p in zip(clones, params):
            c.grad = p.grad
        eager.step(loss=loss)
        assert torch.equal(trainer.grad_norm, eager.grad_norm) and float(trainer.grad_norm) > 0
        assert all(torch.equal(c, p) for c, p in zip(clones, params)), k
    assert len(trainer.buckets) == 2 and trainer.opt_graphs == 2
    assert float(eager.state[clones[0]]["step"]) == 5.0 == float(trainer.optimizer.state[params[0]]["step"])
    # a zero-weight batch: loss 0, the replayed optimizer graph skips
    b = list(trainer.buckets.values())[0]  # the less recently used bucket: batch 0's
    assert len(b) > 3
    b[0].weight.zero_()
    before = [p.detach().clone() for p in params]
    loss, _ = trainer.step(batches[0])
    assert trainer.opt_graphs == 2 and len(trainer.buckets) == 2
    assert float(loss) == 0.0
    assert all(torch.equal(a, p) for a, p in zip(before, params))
    assert float(trainer.optimizer.state[params[0]]["step"]) == 5.0

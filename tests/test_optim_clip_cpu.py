"""Host side of gasfm_amd.optim's device path (no GPU): the C ABI entries of the norm / clip /
capturable-Adam kernels are declared, bound and exported consistently; the pointer tables are cached
per set of gradient tensors, so a repeated step copies nothing; the new keywords are validated."""
import ctypes
import os
import re

import pytest
import torch

from conftest import REPO
from gasfm_amd import _native, optim
from gasfm_amd.optim import Adam

NEW = ("gasfm_grad_sumsq", "gasfm_grad_sumsq_finish", "gasfm_grad_clip", "gasfm_adam_control", "gasfm_adam_step_ctl")


class _Ctl(ctypes.Structure):  # gasfm_adam_ctl (include/gasfm.h)
    _fields_ = [("skip", ctypes.c_int32), ("grad_norm", ctypes.c_float), ("gscale", ctypes.c_float),
                ("step_size", ctypes.c_float), ("inv_bc2_sqrt", ctypes.c_float), ("reserved", ctypes.c_float * 3)]


def test_abi_entries_are_declared_bound_and_exported():
    text = open(os.path.join(REPO, "include", "gasfm.h")).read()
    declared = set(re.findall(r"\b(gasfm_[a-z0-9_]+)\s*\(", text))
    lib = _native.lib()
    for name in NEW:
        assert name in declared and name in _native.exported_symbols() and hasattr(lib, name), name
    fields = re.search(r"typedef struct gasfm_adam_ctl \{(.*?)\} gasfm_adam_ctl;", text, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = [re.sub(r"\[.*\]", "", f.split()[-1]) for f in fields.split(";") if f.strip()]
    assert names == [f[0] for f in _Ctl._fields_]
    assert ctypes.sizeof(_Ctl) == 4 * _native.ADAM_CTL_FLOATS == 32
    modes = {k: int(v) for k, v in re.findall(r"#define GASFM_CLIP_(\w+) (\d+)", text)}
    assert modes == {"NONE": _native.CLIP_MODES[None], "NORM": _native.CLIP_MODES["norm"],
                     "VALUE": _native.CLIP_MODES["value"]}


@pytest.fixture
def launches(monkeypatch):
    """The device path on CPU tensors: the launches are recorded instead of run."""
    calls = []
    for name in ("grad_sumsq", "grad_sumsq_finish", "adam_control", "adam_step_ctl"):
        monkeypatch.setattr(_native, name, lambda *a, _n=name: calls.append((_n, a)))
    monkeypatch.setattr(optim, "_check_param", lambda p: None)
    return calls


def test_tables_are_keyed_by_the_gradient_set(launches, monkeypatch):
    ps = [torch.zeros(n, requires_grad=True) for n in (5, 4097, 3)]
    opt = Adam(ps, capturable=True, grad_clip_mode="norm", grad_clip_th=1.0)
    sets = [[torch.ones(p.numel()) for p in ps] for _ in range(2)]

    def step(k):
        for p, g in zip(ps, sets[k]):
            p.grad = g
        opt.step()

    step(0)
    (tables,) = opt._tables.values()
    assert len(tables) == 1
    step(1)
    assert len(opt._tables) == 1 and len(tables) == 2  # one table per gradient set
    a, b = (t[0] for t in tables.values())
    assert a["tensors"] is not b["tensors"] and a["step"] is b["step"] and a["chunks"] is b["chunks"]
    assert a["tensors"][:, 1].tolist() == [g.data_ptr() for g in sets[0]]
    assert b["tensors"][:, 1].tolist() == [g.data_ptr() for g in sets[1]]
    assert torch.equal(a["tensors"][:, [0, 2, 3, 4]], b["tensors"][:, [0, 2, 3, 4]])
    assert all(opt.state[p]["step"] is a["step"] for p in ps)
    # a repeated step over either set: no copy, no new tensor table
    copies, made = [], []
    copy_, tensor = torch.Tensor.copy_, torch.tensor
    monkeypatch.setattr(torch.Tensor, "copy_", lambda self, *x, **k: copies.append(1) or copy_(self, *x, **k))
    monkeypatch.setattr(torch, "tensor", lambda *x, **k: made.append(1) or tensor(*x, **k))
    del launches[:]
    for k in (0, 1, 1, 0):
        step(k)
    assert copies == [] and made == [] and len(tables) == 2
    used = [c[1][0].data_ptr() for c in launches if c[0] == "adam_step_ctl"]
    assert used == [t["tensors"].data_ptr() for t in (a, b, b, a)]
    assert [c[0] for c in launches][:4] == ["grad_sumsq", "grad_sumsq_finish", "adam_control", "adam_step_ctl"]
    # another subset of the group holds gradients: the tables are rebuilt for it; a table that a
    # captured graph reads (pinned) is retired with everything it points to, not freed
    a["pinned"] = True
    ps[2].grad = None
    opt.step()
    assert len(opt._tables) == 1 and len(next(iter(opt._tables.values()))) == 1
    assert any(t is a for t in opt._retired) and not any(t is b for t in opt._retired)
    new = next(iter(next(iter(opt._tables.values())).values()))[0]
    new["pinned"] = True
    opt.load_state_dict(opt.state_dict())
    assert opt._tables == {} and any(t is new for t in opt._retired)


def test_prepare_builds_without_stepping(launches):
    ps = [torch.zeros(7, requires_grad=True)]
    ps[0].grad = torch.ones(7)
    opt = Adam(ps, track_grad_norm=True)
    opt.prepare()
    assert launches == [] and len(opt._tables) == 1 and opt._ws["partial"].numel() >= 1
    opt.step()
    assert [c[0] for c in launches] == ["grad_sumsq", "grad_sumsq_finish", "adam_control", "adam_step_ctl"]
    assert opt.grad_norm is opt._ws["norm"]


def test_state_dict_holds_one_step_tensor_per_parameter(launches):
    ps = [torch.zeros(3, requires_grad=True), torch.zeros(4, requires_grad=True)]
    for p in ps:
        p.grad = torch.ones_like(p)
    opt = Adam(ps, capturable=True)
    opt.step()
    sd = opt.state_dict()
    s0, s1 = sd["state"][0]["step"], sd["state"][1]["step"]
    assert s0 is not s1 and s0 is not opt.state[ps[0]]["step"]
    assert opt.state[ps[0]]["step"] is opt.state[ps[1]]["step"]  # the live counter stays shared
    assert sd["param_groups"][0]["capturable"] is True
    assert "capturable" not in Adam(ps).state_dict()["param_groups"][0]  # the host path's groups are unchanged


def test_keyword_validation():
    p = torch.zeros(3, requires_grad=True)
    with pytest.raises(ValueError):
        Adam([p], grad_clip_mode="l2", grad_clip_th=1.0)
    with pytest.raises(ValueError):
        Adam([p], grad_clip_mode="norm")
    with pytest.raises(ValueError):
        Adam([p], grad_clip_mode="value", grad_clip_th=0.0)
    with pytest.raises(TypeError):
        Adam([p], lr=torch.tensor(1e-3))  # capturable=False: today's TypeError
    with pytest.raises(TypeError):
        Adam([p], lr=torch.tensor(1e-3), capturable=False)
    Adam([p], lr=torch.tensor(1e-3), capturable=True)
    p.grad = torch.zeros(3)
    with pytest.raises(TypeError):
        Adam([p]).step(loss=torch.tensor(1.0))  # the guard needs the device path
    with pytest.raises(ValueError):
        optim.clip_grad_norm_([p], 1.0, norm_type=1.0)

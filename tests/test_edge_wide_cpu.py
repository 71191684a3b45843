"""The 32 -> 128 edge epilogue without a device: the fp64 restatement and the closed-form backward of
tests/edge_wide_ref.py against autograd of the unfused forward_plan arithmetic (edge_ops.layer_norm_relu,
edge_ops.projection_update, the skip branch's dense.linear) at 1e-12, and the C ABI's new entry points
as gasfm_amd/_abi.py's parser reads them from include/gasfm_edge_wide.h (gasfm_amd/edge_wide/_binding.py)."""
import types

import pytest
import torch

from gasfm_amd import _abi, dense, edge_ops, edge_wide
from gasfm_amd.build import EDGE_WIDE_HEADER
from gasfm_amd.model import GraphAttnSfMLayer

import edge_wide_ref as ref


def _module(mod, **params):
    """mod in fp64 with the given parameters (leaves that collect gradients)."""
    mod = mod.double()
    for k, v in params.items():
        setattr(mod, k, torch.nn.Parameter(v.clone()))
    return mod


def _unfused(c, with_p0):
    """forward_plan's unfused arithmetic on fp64 leaves; returns (P', leaves by name)."""
    Wp = c.Wp if with_p0 else c.Wp[:, :32]
    la = _module(torch.nn.LayerNorm(32, eps=ref.EPS), weight=c.law, bias=c.lab)
    lb = _module(torch.nn.LayerNorm(32, eps=ref.EPS), weight=c.lbw, bias=c.lbb)
    lin_proj = _module(torch.nn.Linear(Wp.shape[1], 128), weight=Wp, bias=c.bp)
    lin_skip = _module(torch.nn.Linear(32, 128), weight=c.Wsk, bias=c.bsk)
    lv = {k: getattr(c, k).clone().requires_grad_(True) for k in ("P", "Sp", "Sv", "Sg")}
    if with_p0:
        lv["P0"] = c.P0.clone().requires_grad_(True)
    edges = types.SimpleNamespace(cam=c.cam, pt=c.pt)
    P_hat = edge_ops.layer_norm_relu(lv["P"], la)
    x_cat = torch.cat([P_hat, lv["P0"]], dim=1) if with_p0 else P_hat
    delta = edge_ops.projection_update(x_cat, lin_proj, lv["Sp"], lv["Sv"], lv["Sg"].view(1, -1), edges)
    skip = dense.linear(edge_ops.layer_norm_relu(lv["P"], lb), lin_skip)
    lv.update(law=la.weight, lab=la.bias, lbw=lb.weight, lbb=lb.bias, Wp=lin_proj.weight, bp=lin_proj.bias,
              Wsk=lin_skip.weight, bsk=lin_skip.bias)
    return skip + delta, lv


@pytest.mark.parametrize("with_p0", [True, False])
@pytest.mark.parametrize("E", [1, 17, 65])
def test_restatements_match_unfused_autograd(E, with_p0):
    c = ref.case(E)
    out, lv = _unfused(c, with_p0)
    torch.testing.assert_close(ref.fwd_of(c, with_p0), out.detach(), rtol=1e-12, atol=1e-12)
    (out * c.dPo).sum().backward()
    closed = ref.bwd_of(c, with_p0)
    assert set(closed) == set(lv) | ({"P0"} - set(lv))
    for k, leaf in lv.items():
        torch.testing.assert_close(closed[k], leaf.grad.reshape(closed[k].shape), rtol=1e-12, atol=1e-12, msg=f"d{k} E={E}")
    assert with_p0 or closed["P0"] is None


def test_big_case_keeps_the_relu_margin():
    c = ref.make_case(3000, 1)
    for g, b in ((c.law, c.lab), (c.lbw, c.lbb)):
        pre = torch.nn.functional.layer_norm(c.P, (32,), g, b, ref.EPS)
        assert float(pre.abs().min()) >= ref.RELU_MARGIN


def test_abi_parses_the_wide_entry_points():
    with open(EDGE_WIDE_HEADER) as f:
        functions, constants, structs = _abi.parse(f.read())
    want = {"gasfm_edge_wide_part_shape": 5, "gasfm_edge_wide_epilogue_fwd": 22, "gasfm_edge_wide_epilogue_bwd": 20,
            "gasfm_segment_rowsum_w": 9}
    assert {k: len(v[1]) for k, v in functions.items()} == want and not constants and not structs
    assert all(restype is not None for restype, _ in functions.values())
    assert edge_wide.functions == functions
    assert not set(want) & set(_abi.functions)  # gasfm.h itself is unchanged: its 32-wide row sum stays as it is
    assert len(_abi.functions["gasfm_segment_rowsum"][1]) == 9


def test_fusable_wide_shapes():
    """fusable_wide() holds for the depth conf's last-block shapes and for no other block."""
    mk = lambda f_in, f_out, skip: GraphAttnSfMLayer(f_in, f_out, 64, 1024, 2048, 32, 32, 64, 1024,  # noqa: E731
                                                     n_feat_skipconn_init_projfeat_in=skip, n_heads=4)
    wide, wide32 = mk(32, 128, 2), mk(32, 128, None)
    assert wide.fusable_wide() and wide32.fusable_wide() and not wide.fusable() and not wide.fusable0()
    assert tuple(wide.projection_feature_update.lin_proj.weight.shape) == (128, 34)
    assert tuple(wide32.projection_feature_update.lin_proj.weight.shape) == (128, 32)
    for other in (mk(32, 32, 2), mk(2, 32, None), mk(32, 64, 2), mk(64, 128, 2)):
        assert not other.fusable_wide()
    hidden = GraphAttnSfMLayer(32, 128, 64, 1024, 2048, 32, 32, 64, 1024, n_feat_skipconn_init_projfeat_in=2, n_heads=4,
                               n_hidden_layers_proj_update=1)
    assert not hidden.fusable_wide()
    no_ln = GraphAttnSfMLayer(32, 128, 64, 1024, 2048, 32, 32, 64, 1024, use_norm_proj_update=False,
                              n_feat_skipconn_init_projfeat_in=2, n_heads=4)
    assert not no_ln.fusable_wide()

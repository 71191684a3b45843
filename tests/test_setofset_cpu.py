"""SetOfSetNet (the DPESFM baseline) on the torch-op composite path against the reference's own
SetOfSetNet (tests/golden/setofset.npz, written by tests/golden/make_golden_setofset.py), the
dpesfm conf preset, the unsupported-conf errors and the ctypes table of the new kernels."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import gasfm_amd
from conftest import REPO, check_fixture_grads, golden
from gasfm_amd import _native, synthetic
from gasfm_amd.conf import Conf, dpesfm_conf
from oracle.weights import deterministic_state_dict

OUT_ATOL, OUT_RTOL = 1e-4, 1e-3

VARIANTS = {
    "shipped": dict(num_features=64),
    "skip": dict(num_features=64, proj_feat_normalization=False, add_skipconn_for_residual_blocks=True,
                 num_blocks=2),
    "depth": dict(num_features=32, depth_head={"enabled": True, "n_feat": 32, "n_hidden_layers": 2}),
}


def fixture_net(f, name, dtype, device="cpu"):
    net = gasfm_amd.SetOfSetNet(dpesfm_conf(**VARIANTS[name]))
    shapes = {k: tuple(int(x) for x in s.split(",")) for k, s in zip(f[f"keys/{name}"], f[f"shapes/{name}"])}
    got = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    assert got == shapes, (sorted(set(got) ^ set(shapes)), [k for k in got if got[k] != shapes.get(k)])
    if name == "shipped":
        sd = {k[3:]: torch.from_numpy(f[k]) for k in f.files if k.startswith("sd/")}
        regen = deterministic_state_dict(net.state_dict(), torch.float32)
        assert all(torch.equal(sd[k], regen[k]) for k in sd)
    else:
        sd = deterministic_state_dict(net.state_dict(), torch.float32)
    net.load_state_dict(sd, strict=True)
    return net.to(dtype).to(device)


def run_linear_loss(net, data, f, dtype):
    dev = data.x.values.device
    pred = net(data)
    loss = (pred["Ps_norm"] * torch.from_numpy(f["cP"]).to(dev, dtype)).sum() \
        + (pred["pts3D"] * torch.from_numpy(f["cX"]).to(dev, dtype)).sum()
    if "depths" in pred:
        loss = loss + (pred["depths"].values * torch.from_numpy(f["cD"]).to(dev, dtype)).sum()
    loss.backward()
    outs = {k: (v.values if k == "depths" else v).detach() for k, v in pred.items()}
    return outs, {k: p.grad for k, p in net.named_parameters()}


def check_against_fixture(f, name, outs, grads, dtype):
    for k, v in outs.items():
        ref = f[f"out/{name}/{k}"]
        tol = dict(atol=OUT_ATOL, rtol=OUT_RTOL) if dtype == torch.float32 else dict(atol=1e-9, rtol=1e-9)
        np.testing.assert_allclose(v.double().cpu().numpy(), ref, err_msg=f"{name} {k}", **tol)
    assert set(outs) == {k.split("/")[2] for k in f.files if k.startswith(f"out/{name}/")}
    check_fixture_grads({f"{name}.{k}": g for k, g in grads.items()}, f, label=f"{dtype} ")


def config1_scene(dtype):
    sc = synthetic.config1()  # built from the dense M as the fixture's scene was (the same torch normalisation)
    data = gasfm_amd.SceneData(torch.from_numpy(sc.dense_M()), torch.from_numpy(sc.Ns()), torch.from_numpy(sc.Ps_gt()),
                               "synthetic_config1")
    data.x.values = data.x.values.to(dtype)
    return data


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("name", list(VARIANTS))
def test_composite_matches_reference_fixture(name, dtype):
    f = golden("setofset.npz")
    net = fixture_net(f, name, dtype)
    outs, grads = run_linear_loss(net, config1_scene(dtype), f, dtype)
    check_against_fixture(f, name, outs, grads, dtype)


def test_shipped_conf_has_40_tensors():
    f = golden("setofset.npz")
    assert len(f["keys/shipped"]) == 40
    sd = gasfm_amd.SetOfSetNet(dpesfm_conf()).state_dict()
    assert len(sd) == 40
    assert tuple(sd["equivariant_blocks.0.layers.1.global_feature_update.lin_view.weight"].shape) == (256, 256)
    assert tuple(sd["equivariant_blocks.0.layers.0.projection_feature_update.lin_proj.weight"].shape) == (256, 2)
    assert "final_global_update.lin_scenepoint.bias" in sd and "view_head.0.weight" in sd
    assert "equivariant_blocks.0.skip_projection.lin_proj.weight" in f["keys/skip"]


# the model section of confs/dpesfm/learning_euc_rhaug-15-20_dpesfm.conf, restated
DPESFM_CONF_TEXT = """
dataset {
  calibrated = true
}
model {
  type = "SetOfSet.SetOfSetNet"
  num_features = 256
  proj_feat_normalization = true
  add_skipconn_for_residual_blocks = false
  num_blocks = 1
  block_size = 3
  pos_emb_n_freq = 0
  depth_head {
    enabled = false
    n_feat = 128
    n_hidden_layers = 2
  }
  view_head {
    enabled = true
    n_hidden_layers = 2
    rot_representation = "quat"
  }
  scenepoint_head {
    enabled = true
    n_hidden_layers = 2
  }
}
"""


def test_dpesfm_conf_equals_the_parsed_conf_text():
    parsed = Conf.parse_string(DPESFM_CONF_TEXT)
    assert parsed.d["model"] == dpesfm_conf().d["model"]
    assert parsed.d["dataset"]["calibrated"] is True and dpesfm_conf().get_bool("dataset.calibrated") is True
    assert dpesfm_conf(num_features=64).get_int("model.num_features") == 64


def test_unsupported_confs_raise():
    with pytest.raises(NotImplementedError):
        gasfm_amd.SetOfSetNet(dpesfm_conf(pos_emb_n_freq=4))
    with pytest.raises(NotImplementedError):
        gasfm_amd.SetOfSetNet(dpesfm_conf(num_features=32), batchnorm=True)
    with pytest.raises(NotImplementedError):
        gasfm_amd.SetOfSetNet(dpesfm_conf(num_features=32, view_head={"enabled": False, "n_hidden_layers": 2}))


def test_gasfm_only_paths_reject_the_baseline():
    net = gasfm_amd.SetOfSetNet(dpesfm_conf(num_features=32))
    from gasfm_amd.batch import forward_batch
    with pytest.raises(TypeError, match="GraphAttnSfMNet"):
        forward_batch(net, [])
    from gasfm_amd.distributed import ShardedGraphAttnSfMNet
    with pytest.raises(TypeError, match="GraphAttnSfMNet"):
        ShardedGraphAttnSfMNet(net)


def test_empty_scene_gives_finite_outputs():
    net = gasfm_amd.SetOfSetNet(dpesfm_conf(num_features=32))
    d0 = gasfm_amd.SceneData.from_sparse(np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, 2), np.float32),
                                         3, 5)
    out = net(d0)
    assert tuple(out["Ps_norm"].shape) == (3, 3, 4) and tuple(out["pts3D"].shape) == (4, 5)
    assert all(bool(torch.isfinite(v).all()) for v in out.values())


NEW_SYMBOLS = ("gasfm_sos_width_ok", "gasfm_sos_row_tile", "gasfm_sos_segment_sum", "gasfm_sos_edge_fwd",
               "gasfm_sos_edge_dx", "gasfm_sos_dw_splits", "gasfm_sos_edge_dw")


def test_new_symbols_are_bound_with_the_header_signature():
    """The existing binding test's rule (tests/test_native_cpu.py) on the set-of-set symbols: every
    one is declared in include/gasfm.h, exported by the library, and bound with the declared arity
    and the ctypes type each C type maps to."""
    scalars = {"int": ctypes.c_int32, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64,
               "float": ctypes.c_float, "double": ctypes.c_double}
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "gasfm.h")).read(), flags=re.S)
    decl = {m.group(1): m for m in re.finditer(r"\b(gasfm_\w+)\s*\(([^;{]*?)\)\s*;", text)}
    lib = _native.lib()
    for name in NEW_SYMBOLS:
        assert name in decl, f"{name} not declared in include/gasfm.h"
        assert hasattr(lib, name), f"{name} not exported"
        restype, argtypes = _native._SIGS[name]
        params = [a.strip() for a in decl[name].group(2).split(",")]
        assert len(params) == len(argtypes), (name, len(params), len(argtypes))
        for i, (p, t) in enumerate(zip(params, argtypes)):
            want = ctypes.c_void_p if "*" in p else scalars[[w for w in p.split() if w != "const"][0]]
            assert want is t, (name, i, p, t)
        ret = re.search(r"([\w \t\*]+)$", text[:decl[name].start(1)]).group(1).strip()
        assert scalars[ret] is restype, (name, ret, restype)
    for k in ("sos_segsum", "sos_edge_fwd", "sos_edge_dx", "sos_edge_dw"):
        assert k in _native.KERNELS and _native.KERNELS[k] < 20


def test_width_rule():
    ok = _native.sos_width_ok
    assert ok(2, 256) and ok(256, 256) and ok(256, 128) and ok(32, 32) and ok(96, 160)
    assert not ok(48, 256) and not ok(256, 48) and not ok(256, 2) and not ok(288, 256) and not ok(4, 32)

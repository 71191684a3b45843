"""The fused depth head without a GPU: its header (include/gasfm_depth_head.h) as the binding reads
it, the exported symbols, the call sites' arity, gasfm.h left alone, what fusable() refuses, and the
unchanged aten path of both networks on CPU tensors."""
import ast
import ctypes
import glob
import os
import subprocess
import types

import torch

import gasfm_amd
from conftest import REPO
from gasfm_amd import _abi, _native, depth_head, synthetic
from gasfm_amd.build import DEPTH_HEAD_HEADER, LIB
from gasfm_amd.conf import dpesfm_conf, small_conf
from gasfm_amd.depth_head import _binding
from gasfm_amd.model import get_linear_layers
from test_abi_cpu import _host_cc

INCLUDE = os.path.join(REPO, "include")
HEAD = {"enabled": True, "n_feat": 128, "n_hidden_layers": 2}


def test_header_parses_and_library_exports_it():
    with open(DEPTH_HEAD_HEADER) as f:
        fns, consts, structs = _abi.parse(f.read())
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert fns == {"gasfm_depth_head_part_shape": (i32, [i64, i32, vp]),
                   "gasfm_depth_head_fwd": (i32, [vp, i64] + 7 * [vp] + [vp]),
                   "gasfm_depth_head_bwd": (i32, [vp, i64] + 9 * [vp] + [vp])}
    assert consts == {} and structs == {}
    assert fns == _binding.functions
    L = ctypes.CDLL(LIB)
    for name in fns:
        assert hasattr(L, name), f"{name} is declared but not exported by libgasfm.so"
    # gasfm.h is left alone: the new entry points live in their own header
    assert len(_abi.functions) == 164 and not any(k.startswith("gasfm_depth_head") for k in _abi.functions)
    # the binding sets the signatures on the library _native loads
    B = _binding.lib()
    assert B is _native.lib() and B.gasfm_depth_head_fwd.argtypes == fns["gasfm_depth_head_fwd"][1]


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "dh.c"
    src.write_text('#include "gasfm_depth_head.h"\nint main(void) { return GASFM_OK; }\n')
    r = subprocess.run([_host_cc(), "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, "-c", str(src), "-o",
                        str(tmp_path / "dh.o")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_call_sites_pass_the_declared_number_of_arguments():
    """The AST count of test_abi_cpu.py, over gasfm_amd/depth_head/ and the new header."""
    bad, seen = [], set()
    for path in sorted(glob.glob(os.path.join(REPO, "gasfm_amd", "depth_head", "*.py"))):
        with open(path) as f:
            tree = ast.parse(f.read(), path)
        for node in ast.walk(tree):
            if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute)
                    and node.func.attr.startswith("gasfm_")):
                continue
            name, where = node.func.attr, f"{os.path.basename(path)}:{node.lineno}"
            assert name in _binding.functions, f"{where}: {name} is not declared in gasfm_depth_head.h"
            assert not any(isinstance(a, ast.Starred) for a in node.args), f"{where}: starred call"
            seen.add(name)
            want = len(_binding.functions[name][1])
            if len(node.args) != want or node.keywords:
                bad.append(f"{where}: {name} passes {len(node.args)} arguments, the header declares {want}")
    assert not bad, "\n".join(bad)
    assert seen == set(_binding.functions)  # the walk sees every wrapper


def test_part_shape_and_empty_calls_need_no_device():
    (ra, ca), (rb, cb) = _binding.part_shape(0, 0), _binding.part_shape(0, 1)
    assert (ra, ca, rb, cb) == (0, 128 * 128 + 128, 0, 128 * 128 + 2 * 128 + 1)
    assert _binding.part_shape(1, 0)[0] == 1 and _binding.part_shape(384, 1)[0] == 1
    assert _binding.part_shape(385, 0)[0] == 2  # 384 rows per backward workgroup before the grid grows
    L = _binding.lib()
    assert L.gasfm_depth_head_fwd(None, 0, None, None, None, None, None, None, None, None) == _native.GASFM_OK
    assert L.gasfm_depth_head_fwd(None, -1, None, None, None, None, None, None, None, None) == _native.GASFM_ERR_INVALID
    assert L.gasfm_depth_head_fwd(None, 5, None, None, None, None, None, None, None, None) == _native.GASFM_ERR_INVALID
    assert L.gasfm_depth_head_bwd(None, 5, *[None] * 10) == _native.GASFM_ERR_INVALID
    assert b"gasfm_depth_head_bwd" in L.gasfm_last_error()


def test_fusable_refuses_everything_but_the_cuda_fp32_128_head():
    head = get_linear_layers(3 * [128] + [1], norm=False)
    P = torch.randn(10, 128)
    assert not depth_head.fusable(head, P)                                   # a CPU tensor (and CPU weights)
    assert not depth_head.fusable(head.double(), P.double())                 # fp64
    assert not depth_head.fusable(get_linear_layers(3 * [64] + [1], norm=False), torch.randn(10, 64))
    assert not depth_head.fusable(get_linear_layers(2 * [128] + [1], norm=False), P)   # one hidden layer
    assert not depth_head.fusable(get_linear_layers(4 * [128] + [1], norm=False), P)   # three
    assert not depth_head.fusable(get_linear_layers(3 * [128] + [1], norm=True), P)
    assert not depth_head.fusable(torch.nn.Linear(128, 1), P) and not depth_head.fusable(head, None)
    try:
        depth_head.apply(head, P)
    except ValueError as e:
        assert "fusable" in str(e)
    else:
        raise AssertionError("apply() on a CPU tensor must raise, not fall back")


def _scene():
    sc = synthetic.config1()
    data = gasfm_amd.SceneData(torch.from_numpy(sc.dense_M()), torch.from_numpy(sc.Ns()), torch.from_numpy(sc.Ps_gt()),
                               "synthetic_config1")
    data.x.values = data.x.values.float()
    return data


def test_setofset_cpu_path_is_the_sequential():
    torch.manual_seed(0)
    net = gasfm_amd.SetOfSetNet(dpesfm_conf(num_features=128, depth_head=HEAD))
    net.composite = True
    seen = {}
    net.depth_head.register_forward_hook(lambda m, i, o: seen.update(P=i[0]))
    data = _scene()
    pred = net(data)
    E = data.x.values.shape[0]
    assert seen["P"].shape == (E, 128) and pred["depths"].values.shape == (E, 1)
    assert torch.equal(pred["depths"].values, net.depth_head(seen["P"]))
    assert [k for k in net.state_dict() if k.startswith("depth_head.")] == [
        f"depth_head.{i}.{k}" for i in (0, 2, 4) for k in ("weight", "bias")]


def test_graph_attn_cpu_outputs_are_the_sequential():
    """GraphAttnSfMNet's blocks have no CPU path: the output stage alone, on stand-in CPU features."""
    torch.manual_seed(0)
    net = gasfm_amd.GraphAttnSfMNet(small_conf(2, depth_head=HEAD))
    data = _scene()
    E, (m, n) = data.x.values.shape[0], data.x.shape[:2]
    P, pts, view = torch.randn(E, 128), torch.randn(n, 64), torch.randn(m, 64)
    net.forward_features = lambda values, edges: (P, pts, view)
    pred = net._forward_outputs(data, data.x.values, types.SimpleNamespace(plans={}), torch.device("cpu"))
    assert pred["depths"].values.shape == (E, 1)
    assert torch.equal(pred["depths"].values, net.depth_head(P))
    assert torch.equal(pred["depths"].indices, data.x.indices)
    assert [k for k in net.state_dict() if k.startswith("depth_head.")] == [
        f"depth_head.{i}.{k}" for i in (0, 2, 4) for k in ("weight", "bias")]

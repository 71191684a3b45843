"""gasfm_amd/_abi.py, the binding read from include/gasfm.h: its struct layouts and constants against
the host C compiler's, the parser's strictness, and the positional arity of every call site."""
import ast
import ctypes
import glob
import os
import shutil
import subprocess

import pytest

from conftest import REPO
from gasfm_amd import _abi, _native

INCLUDE = os.path.join(REPO, "include")


def _host_cc():
    """The clang that ships next to the hipcc gasfm_amd/build.py uses, or the system's cc."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    for cc in (os.path.join(os.path.dirname(hipcc), "amdclang"), shutil.which("cc")):
        if cc and os.access(cc, os.X_OK):
            return cc
    raise AssertionError("no host C compiler (amdclang next to hipcc, or cc)")


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """What the C compiler makes of gasfm.h: {"S name": sizeof, "F name.field": (offset, size),
    "C name": value} for every struct and constant _abi parsed."""
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "gasfm.h"', "int main(void) {"]
    for name, cls in _abi.structs.items():
        lines.append(f'  printf("S {name} %zu\\n", sizeof({name}));')
        for field, _ in cls._fields_:
            lines.append(f'  printf("F {name}.{field} %zu %zu\\n", offsetof({name}, {field}), '
                         f"sizeof((({name}*)0)->{field}));")
    for name in _abi.constants:
        lines.append(f'  printf("C {name} %lld\\n", (long long){name});')
    lines += ["  return 0;", "}"]
    d = tmp_path_factory.mktemp("abi")
    src, exe = str(d / "layout.c"), str(d / "layout")
    with open(src, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([_host_cc(), "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, src, "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    out = {}
    for line in subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines():
        kind, name, *v = line.split()
        out[f"{kind} {name}"] = int(v[0]) if len(v) == 1 else tuple(map(int, v))
    return out


def test_struct_layouts_match_the_compiler(compiled):
    assert len(_abi.structs) == 12
    seen = 0
    for name, cls in _abi.structs.items():
        assert issubclass(cls, ctypes.Structure)
        assert ctypes.sizeof(cls) == compiled[f"S {name}"], name
        for field, _ in cls._fields_:
            f = getattr(cls, field)
            assert (f.offset, f.size) == compiled[f"F {name}.{field}"], f"{name}.{field}"
            seen += 1
    assert seen == sum(k.startswith("F ") for k in compiled)
    # the compiler's own figures for the layouts most exposed to a silent drift
    assert compiled["S gasfm_gchain"] == 272 and compiled["F gasfm_gchain.rows"] == (264, 4)
    assert compiled["S gasfm_union_scene"] == 168
    assert compiled["S gasfm_adam_ctl"] == 32 and compiled["F gasfm_adam_ctl.reserved"] == (20, 12)


def test_constants_match_the_compiler(compiled):
    assert "GASFM_H" not in _abi.constants
    assert {k[2:]: v for k, v in compiled.items() if k.startswith("C ")} == _abi.constants
    assert compiled["C GASFM_K_COUNT"] == 20


def test_native_consumes_the_header():
    """_native's names are the parsed objects, and the derived tables are the ones the header states."""
    assert _native._SIGS is _abi.functions and len(_abi.functions) == 164
    for py, c in (("UnionScene", "gasfm_union_scene"), ("UnionOut", "gasfm_union_out"), ("UnionPad", "gasfm_union_pad"),
                  ("SosTables", "gasfm_sos_tables"), ("_GChain", "gasfm_gchain"), ("_GChainGrads", "gasfm_gchain_grads"),
                  ("_GattProb", "gasfm_gatt_prob")):
        assert getattr(_native, py) is _abi.structs[c]
    C = _abi.constants
    assert len(_native.KERNELS) == 18 and "count" not in _native.KERNELS
    assert all(C["GASFM_K_" + k.upper()] == v for k, v in _native.KERNELS.items())
    assert sorted(_native.KERNELS.values()) == [i for i in range(C["GASFM_K_COUNT"]) if i not in (11, 12)]
    assert _native.TUNING == {"attn_grp_rows": 0, "attn_grp_min_fill": 1, "attn_glds": 2, "attn_wave_cap": 3,
                              "attn_grp_split": 4}
    assert _native.ADAM_CTL_FLOATS * 4 == ctypes.sizeof(_abi.structs["gasfm_adam_ctl"])
    assert (_native.GASFM_OK, _native.GASFM_ERR_INVALID, _native.GASFM_ERR_OOM, _native.GASFM_ERR_HIP,
            _native.GASFM_ERR_UNSUPPORTED) == (0, 1, 2, 3, 4)
    # the name tuples that stay must name fields of the parsed structs
    fields = [f for f, _ in _native.SosTables._fields_]
    groups = _native._SOS_TABLES_IN + _native._SOS_TABLES_I32 + _native._SOS_TABLES_F64 + _native._SOS_TABLES_I64
    assert [f for f in fields if f not in ("M", "N", "E", "S")] == list(groups)
    gc = [f for f, _ in _native._GChain._fields_]
    assert set(_native._GC_W) <= set(gc) and {k + "h" for k in _native._GC_SHADOW} <= set(gc)
    assert [f for f, _ in _native._GChainGrads._fields_] == list(_native._GC_D)


@pytest.mark.parametrize("snippet, word", [
    ("int gasfm_f(size_t n);", "size_t"),                                  # unknown scalar type
    ("typedef struct gasfm_s { long n; } gasfm_s;", "long"),
    ("enum { GASFM_A = 0, GASFM_B };", "GASFM_B"),                          # enum member with no value
    ("int gasfm_f(void (*cb)(int), void* stream);", "gasfm_f"),            # function-pointer parameter
    ("typedef struct gasfm_s { struct { int a; } in; int b; } gasfm_s;", "gasfm_s"),  # nested struct field
    ("typedef struct gasfm_a { int x; } gasfm_a;\ntypedef struct gasfm_s { gasfm_a a; } gasfm_s;", "gasfm_a a"),
    ("unsigned gasfm_f(void);", "gasfm_f"),                                # unknown return type
    ("#define GASFM_X (1 << 4)", "GASFM_X"),                               # a define that is no integer
])
def test_parser_refuses_what_it_does_not_know(snippet, word):
    with pytest.raises(ValueError, match="gasfm.h") as e:
        _abi.parse(snippet)
    assert word in str(e.value)  # the error names the declaration


def test_parser_reads_the_header_grammar():
    vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    fns, consts, structs = _abi.parse("""
        /* a comment with a prototype in it: int gasfm_not(int x); */
        #ifndef GASFM_H
        #define GASFM_H
        #define GASFM_N 7
        enum { GASFM_A = 0, GASFM_B = 3 /* trailing */ };
        typedef struct gasfm_s {
          int32_t G, Kc;
          float eps; /* one */
          const float *W1, *b1, *gM;
          const uint16_t *W1h;
          int64_t E, m, n;
          float reserved[3];
        } gasfm_s;
        const char* gasfm_err(void);
        void gasfm_reset(void);
        int64_t gasfm_count(const gasfm_s* s, const float* const* A, uint32_t* counters,
                            double x, void* stream);
        #endif
    """)
    assert consts == {"GASFM_N": 7, "GASFM_A": 0, "GASFM_B": 3}
    assert fns == {"gasfm_err": (ctypes.c_char_p, []), "gasfm_reset": (None, []),
                   "gasfm_count": (i64, [vp, vp, vp, ctypes.c_double, vp])}
    assert structs["gasfm_s"]._fields_ == [
        ("G", i32), ("Kc", i32), ("eps", f32), ("W1", vp), ("b1", vp), ("gM", vp), ("W1h", vp), ("E", i64),
        ("m", i64), ("n", i64), ("reserved", f32 * 3)]
    assert ctypes.sizeof(structs["gasfm_s"]) == 88


# call sites that unpack a list into the call: their arity is not countable from the source
STARRED_CALLS = {"gasfm_gvec_multi_fwd"}


def test_call_sites_pass_the_declared_number_of_arguments():
    """A miscounted call raises only when its wrapper first runs, on the GPU: count them here."""
    bad, starred, n = [], set(), 0
    for path in sorted(glob.glob(os.path.join(REPO, "gasfm_amd", "*.py"))):
        with open(path) as f:
            tree = ast.parse(f.read(), path)
        for node in ast.walk(tree):
            if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute)
                    and node.func.attr.startswith("gasfm_")):
                continue
            name, where = node.func.attr, f"{os.path.basename(path)}:{node.lineno}"
            assert name in _abi.functions, f"{where}: {name} is not declared in gasfm.h"
            if any(isinstance(a, ast.Starred) for a in node.args):
                starred.add(name)
                continue
            n += 1
            want = len(_abi.functions[name][1])
            if len(node.args) != want or node.keywords:
                bad.append(f"{where}: {name} passes {len(node.args)} arguments, gasfm.h declares {want}")
    assert not bad, "\n".join(bad)
    assert starred == STARRED_CALLS
    assert n >= 150  # the walk sees the wrappers

"""gasfm_gemm_f32 (csrc/gemm_f32.hip): the fp32 MFMA GEMM of the camera-side m x 1024 x 1024
Linear layers (reference code/models/layers.py:292-320, 352-358, 506-511), at m = 1000 (one GPU)
and m = 125 (a camera shard of 8 GPUs), in all three Linear forms (y = x W^T, dx = dy W,
dW = dy^T x) with the fused bias / Cin epilogue.

Reference: the fp64 product.  v_mfma_f32_16x16x4_f32 forms exact products and the kernel sums in
fp32, so the error is fp32 summation error: |C - ref| <= 4 K 2^-24 (|A| |B|) elementwise (+ one
rounding per Cin / bias add) -- the bound a k-ordered fp32 fma chain meets.
"""
import pytest
import torch

import gemm_checks
from gasfm_amd import _native, view_block

pytestmark = pytest.mark.gpu


def check(C, a, b, cin=None, bias=None):
    ad, bd = a.double(), b.double()
    ref = ad @ bd
    bound = 4 * a.shape[1] * 2.0 ** -24 * (ad.abs() @ bd.abs())
    if cin is not None:
        ref = ref + cin.double()
        bound = bound + 2.0 ** -23 * (ref.abs() + cin.double().abs())
    if bias is not None:
        ref = ref + bias.double()
        bound = bound + 2.0 ** -23 * (ref.abs() + bias.double().abs())
    err = (C.double() - ref).abs()
    assert bool((err <= bound + 1e-30).all()), f"max excess {(err - bound).max().item():.3e}"


SHAPES = [(1000, 1024, 1024), (125, 1024, 1024), (128, 1024, 1088), (37, 64, 100), (1, 2048, 1088),
          (64, 4, 8), (130, 260, 36), (7, 32, 1024)]


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_forward_form(device, M, N, K):
    """y = x W^T + b (+ skip): A row-major [M,K], B = W.t() (W [N,K] row-major)."""
    g = torch.Generator(device="cpu").manual_seed(M * 7 + N)
    x = torch.randn(M, K, generator=g).to(device)
    W = (torch.randn(N, K, generator=g) / K ** 0.5).to(device)
    b = torch.randn(N, generator=g).to(device)
    skip = torch.randn(M, N, generator=g).to(device)
    check(_native.gemm_f32(x, W.t()), x, W.t())
    check(_native.gemm_f32(x, W.t(), bias=b), x, W.t(), bias=b)
    check(_native.gemm_f32(x, W.t(), cin=skip, bias=b), x, W.t(), cin=skip, bias=b)
    acc = skip.clone()  # in place: out is cin
    _native.gemm_f32(x, W.t(), cin=acc, out=acc)
    check(acc, x, W.t(), cin=skip)


@pytest.mark.parametrize("M,N,K", [(1000, 1024, 1024), (125, 1024, 1024), (37, 64, 100), (12, 1088, 2048)])
def test_input_grad_form(device, M, N, K):
    """dx = dy W: A = dy [M,K] row-major, B = W [K,N] row-major (n-contiguous)."""
    g = torch.Generator(device="cpu").manual_seed(M + 3 * N)
    dy = torch.randn(M, K, generator=g).to(device)
    W = torch.randn(K, N, generator=g).to(device)
    skip = torch.randn(M, N, generator=g).to(device)
    check(_native.gemm_f32(dy, W), dy, W)
    check(_native.gemm_f32(dy, W, cin=skip), dy, W, cin=skip)


@pytest.mark.parametrize("R,O,I", [(1000, 1024, 1024), (125, 1024, 1024), (100, 64, 36), (2048, 12, 1088), (125, 32, 1024)])
def test_weight_grad_form(device, R, O, I):
    """dW = dy^T x: A = dy.t() (m-contiguous), B = x [R, I] row-major (n-contiguous), K = R."""
    g = torch.Generator(device="cpu").manual_seed(R + O + I)
    dy = torch.randn(R, O, generator=g).to(device)
    x = torch.randn(R, I, generator=g).to(device)
    check(_native.gemm_f32(dy.t(), x), dy.t(), x)


def test_deterministic_and_torch_close(device):
    g = torch.Generator(device="cpu").manual_seed(5)
    a = torch.randn(125, 1024, generator=g).to(device)
    b = torch.randn(1024, 1024, generator=g).to(device)
    c1 = _native.gemm_f32(a, b)
    c2 = _native.gemm_f32(a, b)
    assert torch.equal(c1, c2)
    torch.testing.assert_close(c1, a @ b, rtol=1e-4, atol=1e-3)


def test_rejects_bad_operands(device):
    a = torch.randn(8, 6, device=device)  # K = 6: no float4 runs along k
    with pytest.raises(Exception):
        _native.gemm_f32(a, torch.randn(6, 8, device=device).t().contiguous().t())
    with pytest.raises(ValueError):
        _native.gemm_f32(torch.randn(8, 8, device=device), torch.randn(4, 8, device=device))


# ---- tile edges, strides, K = 0: every call through gemm_checks' guarded output ----------------
# gemm_f32_d_kernel's constants: 64 x 64 tile, 64-wide K chunk (k-contiguous reads clamp to K - 4,
# the last chunk's k >= K are zeroed), tiles remapped over 8 XCDs when their count divides by 8,
# M-tiles in groups of 4.  (M, N, K): ntm x ntn tiles
LARGE = [(1000, 1024, 1000),  # 16 x 16, remap; K % 64 = 40
         (1000, 1000, 1088),  # N % 64 = 40: the column store guard; K % 64 = 0
         (300, 1028, 260),    # 5 x 17 = 85: no remap, ragged last M-group (1 tile), N % 64 = 4, K % 64 = 4
         (380, 760, 68),      # 6 x 12 = 72: remap with a ragged M-group (2 tiles)
         (516, 512, 4)]       # one chunk, the k clamp at 0
LARGE_WGRAD = [(1024, 1024, 999), (300, 1028, 67), (380, 760, 1), (516, 512, 63), (516, 512, 65)]


def _gen(*key):
    return torch.Generator(device="cpu").manual_seed(sum(k * p for k, p in zip(key, (7, 131, 1009, 5))))


@pytest.mark.parametrize("M,N,K", LARGE)
@pytest.mark.parametrize("form", ["fwd", "dgrad", "mixed"])
def test_large_tile_edges(device, form, M, N, K):
    """gemm_f32_d_kernel<AM, BNC> = <0,0> fwd, <0,1> dgrad, <1,0> mixed (P.t() @ W.t())."""
    assert M * N > 262144
    g = _gen(M, N, K, gemm_checks.FORMS.index(form))
    a, b = gemm_checks.operands(form, M, N, K, g, device)
    gemm_checks.run_epilogues(_native.gemm_f32, a, b, g)


@pytest.mark.parametrize("M,N,K", LARGE_WGRAD)
def test_large_tile_edges_wgrad(device, M, N, K):
    """gemm_f32_d_kernel<1,1>: dy.t() @ x, any K (row-contiguous reads clamp to k = K - 1)."""
    assert M * N > 262144
    g = _gen(M, N, K)
    a, b = gemm_checks.operands("wgrad", M, N, K, g, device)
    gemm_checks.run_epilogues(_native.gemm_f32, a, b, g)


@pytest.mark.parametrize("M,N,K", [(512, 512, 64), (512, 516, 64)])
@pytest.mark.parametrize("form", gemm_checks.FORMS)
def test_dispatch_threshold(device, form, M, N, K):
    """M N = 262144 is the last shape of the 32 x 32 kernel, 512 x 516 the first of the 64 x 64 one."""
    g = _gen(M, N, K, gemm_checks.FORMS.index(form))
    a, b = gemm_checks.operands(form, M, N, K, g, device)
    gemm_checks.run_epilogues(_native.gemm_f32, a, b, g)


@pytest.mark.parametrize("M,N,K", [(36, 64, 100), (128, 260, 36)])
def test_small_tile_mixed_form(device, M, N, K):
    """gemm_f32_kernel<AM = 1, BNC = 0>, the one form the Linear products do not use."""
    g = _gen(M, N, K)
    a, b = gemm_checks.operands("mixed", M, N, K, g, device)
    gemm_checks.run_epilogues(_native.gemm_f32, a, b, g)


@pytest.mark.parametrize("form,M,N,K", [("fwd", 37, 64, 100), ("fwd", 130, 260, 36), ("wgrad", 36, 64, 100),
                                        ("mixed", 128, 260, 36), ("fwd", 300, 1028, 260),
                                        ("wgrad", 300, 1028, 67)])
def test_strided_a(device, form, M, N, K):
    """a is a column slice of a wider matrix (sAm = K + 8, or sAk = M + 8 for the m-contiguous forms)."""
    g = _gen(M, N, K, 3)
    a, b = gemm_checks.operands(form, M, N, K, g, device, strided_a=True)
    assert max(a.stride()) == (M if form in ("wgrad", "mixed") else K) + 8
    gemm_checks.run_epilogues(_native.gemm_f32, a, b, g)


@pytest.mark.parametrize("M,N", [(96, 72), (516, 512)])
def test_k_zero(device, M, N):
    """K = 0 on the small- and the large-tile kernel: C = Cin + bias bitwise, zeros without an
    epilogue, nothing outside [M, N] written (the operands' data pointers are null)."""
    g = _gen(M, N)
    a, b = torch.empty(M, 0, device=device), torch.empty(0, N, device=device)
    bias = torch.randn(N, generator=g).to(device)
    cin = torch.randn(M, N, generator=g).to(device)
    z = gemm_checks.run_checked(_native.gemm_f32, a, b)
    assert torch.equal(z, torch.zeros(M, N, device=device))
    assert torch.equal(gemm_checks.run_checked(_native.gemm_f32, a, b, bias=bias), bias.expand(M, N))
    assert torch.equal(gemm_checks.run_checked(_native.gemm_f32, a, b, cin=cin, bias=bias), cin + bias)
    assert torch.equal(gemm_checks.run_checked(_native.gemm_f32, a, b, cin=cin, alias=True), cin)


def test_empty_m_and_n(device):
    b = torch.randn(40, 72, device=device)
    assert _native.gemm_f32(torch.empty(0, 40, device=device), b).shape == (0, 72)
    assert _native.gemm_f32(torch.randn(96, 40, device=device), torch.empty(40, 0, device=device)).shape == (96, 0)


@pytest.mark.parametrize("form,M,N,K", [("fwd", 300, 1028, 260), ("wgrad", 300, 1028, 260), ("fwd", 130, 260, 36)])
def test_nan_isolation(device, form, M, N, K):
    g = _gen(M, N, K, 9)
    a, b = gemm_checks.operands(form, M, N, K, g, device)
    gemm_checks.check_nan_isolation(_native.gemm_f32, a, b)


def test_view_block_dispatch(device, monkeypatch):
    """view_block._mm hands every product to gemm_f32 under GASFM_VIEW_GEMM=hip, and the weight
    gradient above SMALLM_ROWS rows under GASFM_WGRAD_GEMM=hip (bitwise equal to direct calls)."""
    g = _gen(11)
    x = torch.randn(1000, 512, generator=g).to(device)
    dy = torch.randn(1000, 1024, generator=g).to(device)
    W = (torch.randn(1024, 512, generator=g) / 32).to(device)
    b = torch.randn(1024, generator=g).to(device)
    skip = torch.randn(1000, 1024, generator=g).to(device)
    assert x.shape[0] > view_block.SMALLM_ROWS
    monkeypatch.setattr(view_block, "FP32_GEMM", "torch")
    monkeypatch.setattr(view_block, "WGRAD_HIP", True)
    assert torch.equal(view_block._mm(dy.t(), x), _native.gemm_f32(dy.t(), x))
    monkeypatch.setattr(view_block, "WGRAD_HIP", False)
    monkeypatch.setattr(view_block, "FP32_GEMM", "hip")
    assert torch.equal(view_block._mm(x, W.t(), cin=skip, bias=b), _native.gemm_f32(x, W.t(), cin=skip, bias=b))
    assert torch.equal(view_block._mm(dy, W), _native.gemm_f32(dy, W))
    assert torch.equal(view_block._mm(dy.t(), x), _native.gemm_f32(dy.t(), x))
    acc = skip.clone()
    assert view_block._mm(x, W.t(), cin=acc, out=acc) is acc
    assert torch.equal(acc, _native.gemm_f32(x, W.t(), cin=skip))

"""The small-row-count fp32 GEMMs (csrc/gemm_smallm.hip, gasfm_gemm_f32_smallm) against an fp64 torch
reference: the three products of the camera-side Linear layers on a camera-sharded rank (125 rows
at config 4 on 8 GPUs) and a training batch (~60 rows), with the fused bias / skip epilogue and the
in-place skip.  Tolerance (fp32 MFMA, k-ordered fp32 sums over K <= 1024 vs fp64):
|d| <= 1e-4 |ref|_max + 1e-6, the products' inputs being O(1), and (gemm_checks.run_checked) the
elementwise fp32 summation bound 4 K 2^-24 (|A| |B|) into a NaN-guarded, strided output.  The
view-chain dispatch (view_block._mm) is checked to take this kernel at m <= GASFM_SMALLM_ROWS.
"""
import pytest
import torch

import gemm_checks
from gasfm_amd import _native, view_block

pytestmark = pytest.mark.gpu


def _close(got, ref):
    ref = ref.double()
    err = float((got.double() - ref).abs().max())
    assert err <= 1e-4 * float(ref.abs().max()) + 1e-6, err


@pytest.mark.parametrize("M", [1, 17, 60, 125, 256])
@pytest.mark.parametrize("K", [128, 1024])
def test_xwt_and_xw(device, M, K):
    g = torch.Generator(device=device).manual_seed(M * 7 + K)
    N = 1024
    x = torch.randn(M, K, generator=g, device=device)
    W = torch.randn(N, K, generator=g, device=device) / K ** 0.5
    b = torch.randn(N, generator=g, device=device)
    skip = torch.randn(M, N, generator=g, device=device)
    y = _native.gemm_f32_smallm(x, W.t())
    assert y is not None
    _close(y, x.double() @ W.double().t())
    y = _native.gemm_f32_smallm(x, W.t(), bias=b)
    _close(y, x.double() @ W.double().t() + b.double())
    ref = skip.double() + x.double() @ W.double().t()
    y = _native.gemm_f32_smallm(x, W.t(), cin=skip, out=skip)  # in place, as ViewTailFn's MLP
    assert y is skip
    _close(y, ref)
    # dx = dy W with W [K_out = K, N]
    W2 = torch.randn(K, N, generator=g, device=device) / K ** 0.5
    y = _native.gemm_f32_smallm(x, W2)
    _close(y, x.double() @ W2.double())
    # the same products into a guarded, strided output at the elementwise bound
    gemm_checks.run_epilogues(SM, x, W.t(), _gen(M, K))
    assert gemm_checks.run_checked(SM, x, W2) is not None


@pytest.mark.parametrize("K", [1, 16, 60, 125, 256])
def test_wgrad(device, K):
    g = torch.Generator(device=device).manual_seed(K)
    dy = torch.randn(K, 1024, generator=g, device=device)
    x = torch.randn(K, 512, generator=g, device=device)
    y = _native.gemm_f32_smallm(dy.t(), x)
    assert y is not None and y.shape == (1024, 512)
    _close(y, dy.double().t() @ x.double())
    assert gemm_checks.run_checked(SM, dy.t(), x) is not None


def test_unsupported_forms_fall_back(device):
    a = torch.randn(8, 100, device=device)  # K not a multiple of the K-slicing
    assert _native.gemm_f32_smallm(a, torch.randn(64, 100, device=device).t()) is None
    a = torch.randn(8, 64, device=device)
    assert _native.gemm_f32_smallm(a, torch.randn(64, 48, device=device)) is None  # N % 32 != 0
    assert _native.gemm_f32_smallm(a, torch.randn(64, 64, device=device), bias=torch.zeros(64, device=device)) is None


def test_view_chain_dispatch(device):
    """view_block._mm takes the small-M kernels for the three products at m = 125 (dispatch seen
    through the results' bitwise equality with direct calls)."""
    g = torch.Generator(device=device).manual_seed(3)
    m, D = 125, 1024
    h = torch.randn(m, D, generator=g, device=device)
    Wm = torch.randn(D, D, generator=g, device=device) / 32
    dv = torch.randn(m, D, generator=g, device=device)
    assert m <= view_block.SMALLM_ROWS
    assert torch.equal(view_block._mm(h, Wm.t()), _native.gemm_f32_smallm(h, Wm.t()))
    assert torch.equal(view_block._mm(dv, Wm), _native.gemm_f32_smallm(dv, Wm))
    assert torch.equal(view_block._mm(dv.t(), h), _native.gemm_f32_smallm(dv.t(), h))


# ---- every template instance, tile boundaries, strides: through gemm_checks' guarded output ----
# gemm_sm_rows_kernel<MODE, KQ>: 16 x 32 tile, KQ = K / 128 in {1, 2, 4, 8, 16};
# gemm_sm_wgrad_kernel<KU>: 16 x 128 per workgroup, KU = 1, 2, 4, 8, 16 for ceil(K / 16) <= KU.
SM = _native.gemm_f32_smallm


def _gen(*key):
    return torch.Generator(device="cpu").manual_seed(sum(k * p for k, p in zip(key, (7, 131, 1009, 5))))


def _close_after(a, b):
    p = a.double() @ b.double()

    def after(C, cin, bias):
        ref = p
        if cin is not None:
            ref = ref + cin.double()
        if bias is not None:
            ref = ref + bias.double()
        _close(C, ref)
    return after


def _modes01(device, M, N, K, strided_a=False):
    g = _gen(M, N, K, int(strided_a))
    a, b = gemm_checks.operands("fwd", M, N, K, g, device, strided_a=strided_a)  # mode 0, every epilogue
    gemm_checks.run_epilogues(SM, a, b, g, after=_close_after(a, b))
    a, b = gemm_checks.operands("dgrad", M, N, K, g, device, strided_a=strided_a)  # mode 1
    y = gemm_checks.run_checked(SM, a, b)
    assert y is not None
    _close(y, a.double() @ b.double())


@pytest.mark.parametrize("K", [128, 256, 512, 1024, 2048])
@pytest.mark.parametrize("N", [32, 1024])
def test_rows_every_kq(device, N, K):
    """gemm_sm_rows_kernel<0, KQ> and <1, KQ> for KQ = K / 128 = 1, 2, 4, 8, 16; N = 32 is one tile column."""
    _modes01(device, 17, N, K)


@pytest.mark.parametrize("M", [1, 15, 16, 17, 31, 32, 33, 125, 256])
@pytest.mark.parametrize("N,K", [(32, 128), (96, 2048)])
def test_rows_tile_boundary(device, M, N, K):
    """M below, on and above the 16-row tile."""
    _modes01(device, M, N, K)


@pytest.mark.parametrize("M,N,K", [(17, 32, 128), (33, 96, 512)])
def test_rows_strided_a(device, M, N, K):
    """lda = K + 8: a column slice of a wider activation."""
    _modes01(device, M, N, K, strided_a=True)


def _fallback_ok(device, a, b, cin=None, bias=None):
    """Not this kernel's form: gemm_f32_smallm returns None, view_block._mm still computes it."""
    assert gemm_checks.run_checked(SM, a, b, cin=cin, bias=bias) is None
    assert a.shape[0] <= view_block.SMALLM_ROWS
    y = view_block._mm(a, b, cin=cin, bias=bias)
    ref, bound = gemm_checks.reference(a, b, cin, bias)
    gemm_checks.assert_within(y, ref, bound, what="view_block._mm fallback")


@pytest.mark.parametrize("form,M,N,K", [("fwd", 17, 32, 4096), ("dgrad", 17, 32, 4096), ("fwd", 17, 32, 192),
                                        ("dgrad", 17, 32, 192), ("fwd", 17, 48, 128), ("dgrad", 17, 48, 128)])
def test_rows_not_mine(device, form, M, N, K):
    g = _gen(M, N, K)
    _fallback_ok(device, *gemm_checks.operands(form, M, N, K, g, device))


def test_rows_misaligned_and_mode1_epilogue(device):
    M, N, K = 17, 32, 128
    g = _gen(M, N, K, 2)
    _, b = gemm_checks.operands("fwd", M, N, K, g, device)
    a = torch.randn(M * K + 1, generator=g).to(device)[1:].view(M, K)  # 4 bytes off a 16-byte boundary
    assert a.data_ptr() % 16 == 4
    _fallback_ok(device, a, b)
    a, b = gemm_checks.operands("dgrad", M, N, K, g, device)
    bias = torch.randn(N, generator=g).to(device)
    cin = torch.randn(M, N, generator=g).to(device)
    _fallback_ok(device, a, b, bias=bias)
    _fallback_ok(device, a, b, cin=cin)


@pytest.mark.parametrize("K", [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256])
@pytest.mark.parametrize("I,J", [(16, 128), (48, 384), (1024, 512)])
def test_wgrad_every_ku(device, I, J, K):
    """gemm_sm_wgrad_kernel<KU>, both sides of every KU boundary, with dy plain and a column slice
    of a wider matrix (lda = I + 8)."""
    for strided in (False, True):
        g = _gen(I, J, K, int(strided))
        a, b = gemm_checks.operands("wgrad", I, J, K, g, device, strided_a=strided)
        y = gemm_checks.run_checked(SM, a, b)
        assert y is not None
        _close(y, a.double() @ b.double())


@pytest.mark.parametrize("I,J,K", [(16, 128, 257), (8, 128, 16), (16, 64, 16)])
def test_wgrad_not_mine(device, I, J, K):
    g = _gen(I, J, K)
    a, b = gemm_checks.operands("wgrad", I, J, K, g, device)
    assert gemm_checks.run_checked(SM, a, b) is None


def test_nan_isolation(device):
    g = _gen(1)
    gemm_checks.check_nan_isolation(SM, *gemm_checks.operands("fwd", 17, 32, 128, g, device))
    # mode 2: the NaN sits in the last valid k row (K = 17 of KU = 2's 32); the zeroed rows past K
    # re-read that row and must not carry it anywhere else
    gemm_checks.check_nan_isolation(SM, *gemm_checks.operands("wgrad", 16, 128, 17, g, device))

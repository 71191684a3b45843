"""Shared checks of the hand-written GEMMs (csrc/gemm_f32.hip, gemm_bf16.hip, gemm_smallm.hip).

Every call writes into a view of a NaN-filled, padded buffer, so an element the kernel skipped
(still NaN) and an element it wrote outside [M, N] (a guard no longer NaN) both fail, whatever the
caching allocator left in the block.  The output's row stride (N + 8), a separate Cin's (N + 4) and
the operands' (builders below) differ from the plain N / K of a fresh tensor.  The view starts at
row 1, column 0: include/gasfm.h asks for 16-byte aligned row starts, which N % 4 == 0 keeps.

Reference: the fp64 product (of the bf16-rounded operands for gemm_bf16).  The MFMA products are
exact and the sums fp32, so for ANY order of the K fused multiply-adds
    |C - ref| <= 4 K 2^-24 (|A| |B|)   elementwise,
plus 2^-23 (|ref| + |addend|) per Cin / bias add, plus 1e-30.  Derived, not measured; the same
bound for all three kernels.
"""
import torch

PAD_ROWS, PAD_COLS, CIN_PAD = 1, 8, 4


def bf16_round(x):
    return x.to(torch.bfloat16).to(torch.float32)


def products(a, b, round_operands=False):
    """(A B, |A| |B|) in fp64; compute once and pass as ``prods`` to the calls that share a, b."""
    ad, bd = (bf16_round(a), bf16_round(b)) if round_operands else (a, b)
    ad, bd = ad.double(), bd.double()
    return ad @ bd, ad.abs() @ bd.abs()


def reference(a, b, cin=None, bias=None, round_operands=False, prods=None):
    """(fp64 reference, elementwise bound) of a @ b (+ cin) (+ bias)."""
    ref, ab = prods if prods is not None else products(a, b, round_operands)
    bound = 4 * a.shape[1] * 2.0 ** -24 * ab
    for add in (cin, bias):
        if add is not None:
            ref = ref + add.double()
            bound = bound + 2.0 ** -23 * (ref.abs() + add.double().abs())
    return ref, bound + 1e-30


def assert_within(C, ref, bound, nan_row=None, nan_col=None, what=""):
    """C finite and within bound of ref everywhere, except exactly row nan_row / column nan_col,
    which must be NaN throughout."""
    nan = torch.isnan(C)
    want = torch.zeros_like(nan)
    if nan_row is not None:
        want[nan_row, :] = True
    if nan_col is not None:
        want[:, nan_col] = True
    assert torch.equal(nan, want), (
        f"{what}: {int((nan & ~want).sum())} unexpected NaN (unwritten or poisoned), "
        f"{int((want & ~nan).sum())} missing NaN; first at {(nan ^ want).nonzero()[:4].tolist()}")
    ok = ~want
    assert bool(torch.isfinite(C[ok]).all()), f"{what}: non-finite output"
    excess = ((C.double() - ref).abs() - bound)[ok]
    if excess.numel():
        assert bool((excess <= 0).all()), f"{what}: max excess over the bound {excess.max().item():.3e}"


def _guarded(M, N, device):
    buf = torch.full((M + 2 * PAD_ROWS, N + PAD_COLS), float("nan"), dtype=torch.float32, device=device)
    return buf, buf[PAD_ROWS:PAD_ROWS + M, :N]


def _guards_intact(buf, M, N, what):
    g = torch.isnan(buf)
    g[PAD_ROWS:PAD_ROWS + M, :N] = True
    assert bool(g.all()), f"{what}: wrote outside [M, N]; first at (buffer row, col) {(~g).nonzero()[:4].tolist()}"


def _call(fn, a, b, cin, bias, alias):
    """fn into a guarded view; (buffer, view) or None when fn declines the form."""
    M, N = a.shape[0], b.shape[1]
    buf, out = _guarded(M, N, a.device)
    cin_arg = None
    if cin is not None:
        if alias:
            out.copy_(cin)
            cin_arg = out
        else:  # its own buffer and row stride
            cin_arg = torch.empty((M, N + CIN_PAD), dtype=torch.float32, device=a.device)[:, :N]
            cin_arg.copy_(cin)
    got = fn(a, b, cin=cin_arg, bias=bias, out=out)
    if got is None:
        return None
    assert got is out
    return buf, out


def run_checked(fn, a, b, cin=None, bias=None, round_operands=False, alias=False, prods=None):
    """fn(a, b, cin=, bias=, out=) into a guarded, strided output; the result against the fp64
    reference at the elementwise bound, the guards untouched.  alias: cin is out (in place).
    Returns the output view, or None when fn returns None (gemm_f32_smallm's "not mine")."""
    assert not alias or cin is not None
    M, N, K = a.shape[0], b.shape[1], a.shape[1]
    what = f"[{M},{N},{K}] cin={cin is not None} bias={bias is not None} alias={alias}"
    r = _call(fn, a, b, cin, bias, alias)
    if r is None:
        return None
    buf, out = r
    ref, bound = reference(a, b, cin, bias, round_operands, prods)
    _guards_intact(buf, M, N, what)
    assert_within(out, ref, bound, what=what)
    return out


def run_epilogues(fn, a, b, gen, round_operands=False, after=None):
    """run_checked without an epilogue, with bias, with cin + bias (separate cin) and with cin
    aliasing out, on one shared reference.  after(out, cin, bias): a further check per variant."""
    M, N = a.shape[0], b.shape[1]
    bias = torch.randn(N, generator=gen).to(a.device)
    cin = torch.randn(M, N, generator=gen).to(a.device)
    prods = products(a, b, round_operands)
    for c, bs, al in ((None, None, False), (None, bias, False), (cin, bias, False), (cin, None, True)):
        out = run_checked(fn, a, b, cin=c, bias=bs, round_operands=round_operands, alias=al, prods=prods)
        assert out is not None
        if after is not None:
            after(out, c, bs)


def check_nan_isolation(fn, a, b, round_operands=False):
    """A NaN in a[M-1, K-1] must make exactly row M-1 of the result NaN, one in b[K-1, N-1] exactly
    column N-1: the last valid element sits next to every clamped out-of-range read (rows >= M,
    columns >= N, k >= K), so a clamped value that reaches a stored element, or a k mask on the
    wrong lane, shows as a NaN elsewhere or as a finite value in that row / column."""
    M, N, K = a.shape[0], b.shape[1], a.shape[1]
    ref, bound = reference(a, b, round_operands=round_operands)
    for t, idx, row, col in ((a, (M - 1, K - 1), M - 1, None), (b, (K - 1, N - 1), None, N - 1)):
        keep = t[idx].clone()
        t[idx] = float("nan")
        try:
            r = _call(fn, a, b, None, None, False)
        finally:
            t[idx] = keep
        assert r is not None
        buf, out = r
        what = f"[{M},{N},{K}] NaN in {'a' if t is a else 'b'}"
        _guards_intact(buf, M, N, what)
        assert_within(out, ref, bound, nan_row=row, nan_col=col, what=what)


FORMS = ("fwd", "dgrad", "wgrad", "mixed")


def operands(form, M, N, K, gen, device, strided_a=False):
    """(a [M,K], b [K,N]) views of row-major fp32 tensors in one of the four stride forms:
      fwd    x @ W.t()      a k-contiguous, b k-contiguous   (K % 4 == 0)
      dgrad  dy @ W         a k-contiguous, b n-contiguous   (K % 4 == 0, N % 4 == 0)
      wgrad  dy.t() @ x     a m-contiguous, b n-contiguous   (M % 4 == 0, N % 4 == 0, any K)
      mixed  P.t() @ W.t()  a m-contiguous, b k-contiguous   (M % 4 == 0, K % 4 == 0)
    strided_a: a is a column slice [:, 4:4+c] of a matrix 8 columns wider (row stride c + 8)."""
    a_mcontig = form in ("wgrad", "mixed")
    r, c = (K, M) if a_mcontig else (M, K)
    if strided_a:
        A = torch.randn(r, c + 8, generator=gen).to(device)[:, 4:4 + c]
    else:
        A = torch.randn(r, c, generator=gen).to(device)
    a = A.t() if a_mcontig else A
    scale = max(K, 1) ** -0.5
    if form in ("fwd", "mixed"):
        b = (torch.randn(N, K, generator=gen) * scale).to(device).t()
    else:
        b = (torch.randn(K, N, generator=gen) * scale).to(device)
    assert a.shape == (M, K) and b.shape == (K, N)
    return a, b

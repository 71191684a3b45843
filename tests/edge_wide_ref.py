"""fp64 torch restatements of the 32 -> 128 edge epilogue (csrc/edge_wide.hip) and of its backward in
closed form, with the shared inputs of tests/test_edge_wide_cpu.py and tests/test_gpu_edge_wide.py (a
plain module like relu_edge.py, not a fixture).  Nothing here needs a device."""
import functools
import types

import torch
import torch.nn.functional as F

from relu_edge import RELU_MARGIN, off_relu_edge

EPS = 1e-5
SCALE = 0.25
WO = 128
M_TAB, N_TAB = 5, 7


def _ln_relu(P, g, b, eps):
    return F.relu(F.layer_norm(P, P.shape[1:], g, b, eps))


def wide_ref(P, P0, cam, pt, law, lab, lbw, lbb, Wp, bp, Wsk, bsk, Sp, Sv, Sg, eps=EPS):
    """P' = Wsk relu(LN_b(P)) + bsk + (Wp [relu(LN_a(P)) | P0] + bp + Sp[pt] + Sv[cam] + Sg) / 4."""
    pa, pb = _ln_relu(P, law, lab, eps), _ln_relu(P, lbw, lbb, eps)
    x = pa if P0 is None else torch.cat([pa, P0], 1)
    return pb @ Wsk.T + bsk + SCALE * (x @ Wp.T + bp + Sp[pt] + Sv[cam] + Sg.reshape(-1))


def wide_bwd_ref(P, P0, cam, pt, law, lab, lbw, lbb, Wp, Wsk, dPo, m, n, eps=EPS):
    """The backward in closed form: every gradient of wide_ref for the output gradient dPo."""
    mean = P.mean(1, keepdim=True)
    rstd = ((P - mean).pow(2).mean(1, keepdim=True) + eps).rsqrt()
    xh = (P - mean) * rstd
    prea, preb = xh * law + lab, xh * lbw + lbb
    ha, hb = prea.clamp_min(0), preb.clamp_min(0)
    dya = (SCALE * dPo @ Wp[:, :32]) * (prea > 0)
    dyb = (dPo @ Wsk) * (preb > 0)

    def ln_bwd(dy, w):
        gv = dy * w
        return rstd * (gv - gv.mean(1, keepdim=True) - xh * (gv * xh).mean(1, keepdim=True))

    x = ha if P0 is None else torch.cat([ha, P0], 1)
    z = lambda rows: torch.zeros(rows, dPo.shape[1], dtype=dPo.dtype)  # noqa: E731
    return dict(P=ln_bwd(dya, law) + ln_bwd(dyb, lbw), P0=None if P0 is None else SCALE * dPo @ Wp[:, 32:],
                Wp=SCALE * dPo.T @ x, bp=SCALE * dPo.sum(0), Wsk=dPo.T @ hb, bsk=dPo.sum(0),
                law=(dya * xh).sum(0), lab=dya.sum(0), lbw=(dyb * xh).sum(0), lbb=dyb.sum(0),
                Sv=SCALE * z(m).index_add(0, cam, dPo), Sp=SCALE * z(n).index_add(0, pt, dPo), Sg=SCALE * dPo.sum(0))


def _r(g, *shape, scale=1.0, shift=0.0):
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale + shift


def nudge_off_edge(P, params, eps=EPS):
    """P with the few elements whose pre-activation under any of the (gamma, beta) pairs lies within
    RELU_MARGIN of 0 moved by 0.01 (sizes with too many rows for a per-column shift of beta)."""
    for _ in range(50):
        bad = torch.zeros_like(P, dtype=torch.bool)
        for g, b in params:
            bad |= F.layer_norm(P, P.shape[1:], g, b, eps).abs() < RELU_MARGIN
        if not bool(bad.any()):
            return P
        P = P + 0.01 * bad
    raise AssertionError("pre-activations stay on the ReLU edge")


def make_case(E, seed, cam=None, pt=None, m=M_TAB, n=N_TAB):
    """fp64 inputs at E edges; cam / pt random indices into m / n rows (index 0 in the last row) unless
    given.  Both LayerNorms' pre-activations keep RELU_MARGIN from 0."""
    g = torch.Generator().manual_seed(seed)
    c = types.SimpleNamespace(E=E, m=m, n=n)
    c.P, c.P0 = _r(g, E, 32, scale=1.5, shift=0.2), _r(g, E, 2)
    c.law, c.lab = _r(g, 32, scale=0.3, shift=1), _r(g, 32, scale=0.2)
    c.lbw, c.lbb = _r(g, 32, scale=0.3, shift=1), _r(g, 32, scale=0.2)
    if 0 < E <= 1000:
        c.lab, c.lbb = off_relu_edge(c.P, c.law, c.lab, EPS), off_relu_edge(c.P, c.lbw, c.lbb, EPS)
    elif E:
        c.P = nudge_off_edge(c.P, [(c.law, c.lab), (c.lbw, c.lbb)])
    c.Wp, c.bp = _r(g, WO, 34, scale=0.2), _r(g, WO, scale=0.1)
    c.Wsk, c.bsk = _r(g, WO, 32, scale=0.2), _r(g, WO, scale=0.1)
    c.Sp, c.Sv, c.Sg = _r(g, n, WO), _r(g, m, WO), _r(g, WO)
    if cam is None:
        cam, pt = torch.randint(0, m, (E,), generator=g), torch.randint(0, n, (E,), generator=g)
        if E:
            cam[-1] = pt[-1] = 0
    c.cam, c.pt = cam, pt
    c.dPo = _r(g, E, WO)
    return c


@functools.lru_cache(maxsize=None)
def case(E):
    return make_case(E, 9000 + E)


def fwd_of(c, with_p0):
    return wide_ref(c.P, c.P0 if with_p0 else None, c.cam, c.pt, c.law, c.lab, c.lbw, c.lbb,
                    c.Wp if with_p0 else c.Wp[:, :32], c.bp, c.Wsk, c.bsk, c.Sp, c.Sv, c.Sg)


def bwd_of(c, with_p0):
    return wide_bwd_ref(c.P, c.P0 if with_p0 else None, c.cam, c.pt, c.law, c.lab, c.lbw, c.lbb,
                        c.Wp if with_p0 else c.Wp[:, :32], c.Wsk, c.dPo, c.m, c.n)


@functools.lru_cache(maxsize=None)
def fwd_ref(E, with_p0):
    return fwd_of(case(E), with_p0)

"""References of the flow diagnostics (include/lns.h "flow diagnostics"; lns_op_flow_stats, lns_op_vorticity,
lns_rollout_eval_flow), in torch, on whatever device the inputs live on.

`statement32`: the statement of include/lns.h as explicit unfused fp32 ops in the written order -- one torch op per written
operator, the plane sums in the order of the metric kernels (`sums32`), quotients and square roots the correctly rounded ones,
the constants device tensors.  The kernel is held to it bit for bit.  `stats64`: every output in float64 from the same fp32
inputs (the denormalisation's constants and the spacings rounded to fp32 first, as the specs hold them).  `stats32_torch`: the
same quantities from torch's own fp32 reductions -- the `own` of the project's rule max(2e-7, 3 x own).  `vorticity32` /
`vorticity64`: the pointwise field.  `counts`: the vorticity histogram by the numpy bin rule of the field statistics.

Layouts: y_hat, y [B, T, C, H, W] -> [B, T, 12] in the order of NAMES; vorticity [B, T, H, W].  `bc` = (bc_y, bc_x), 0 periodic,
1 wall.  `norm`: the keyword arguments of lns_amd.engine.eval_spec."""
import numpy as np
import torch

from ensemble_score_reference import _div32, _norm, _sqrt32, denorm
from field_stats_reference import bin_rule, sums32

NAMES = ("ke_P", "ke_Q", "ens_P", "ens_Q", "div_P", "div_Q", "vort_err", "vort_cos", "vel_err", "maxvort_P", "maxvort_Q", "maxdiv_P")
PERIODIC, WALL = 0, 1


def host_constants(d):
    """(rc, re) of an axis with spacing d, as the host forms them: d is the fp32 the spec holds."""
    d = float(np.float32(d))
    return float(np.float32(1.0 / (2.0 * d))), float(np.float32(1.0 / d))


def deriv(f, dim, wall, d, dtype=torch.float32):
    """The derivative of the statement along `dim` (-2: y, -1: x) of f [..., H, W]: the difference rounded first, then the
    product.  In float64 the constants are 1 / (2 d) and 1 / d of the fp32 spacing."""
    n = f.shape[dim]
    if n == 1:
        return torch.zeros_like(f)
    if dtype == torch.float32:
        rc, re = (torch.tensor(c, dtype=torch.float32, device=f.device) for c in host_constants(d))
    else:
        d64 = float(np.float32(d))
        rc, re = (torch.tensor(c, dtype=torch.float64, device=f.device) for c in (1.0 / (2.0 * d64), 1.0 / d64))
    if not wall:
        diff = torch.roll(f, -1, dim) - torch.roll(f, 1, dim)
        return diff * rc
    out = torch.empty_like(f)
    sl = [slice(None)] * f.dim()

    def at(s):
        k = list(sl)
        k[dim] = s
        return tuple(k)
    if n > 2:
        diff = f[at(slice(2, None))] - f[at(slice(None, -2))]
        out[at(slice(1, -1))] = diff * rc
    edge = f[at(slice(1, 2))] - f[at(slice(0, 1))]
    out[at(slice(0, 1))] = edge * re
    edge = f[at(slice(n - 1, n))] - f[at(slice(n - 2, n - 1))]
    out[at(slice(n - 1, n))] = edge * re
    return out


def pixel_fields(x, u, v, dx, dy, bc, norm, dtype=torch.float32):
    """x [B, T, C, H, W] normalised -> (U, V, w, dv), each [B, T, H, W] in `dtype`."""
    D = denorm(x, norm, dtype)
    U, V = D[:, :, u], D[:, :, v]
    dxU, dxV = deriv(U, -1, bc[1] == WALL, dx, dtype), deriv(V, -1, bc[1] == WALL, dx, dtype)
    dyU, dyV = deriv(U, -2, bc[0] == WALL, dy, dtype), deriv(V, -2, bc[0] == WALL, dy, dtype)
    return U, V, dxV - dyU, dxU + dyV


def vorticity32(x, u=0, v=1, dx=1.0, dy=1.0, bc=(PERIODIC, PERIODIC), **norm):
    return pixel_fields(x, u, v, dx, dy, bc, norm)[2]


def vorticity64(x, u=0, v=1, dx=1.0, dy=1.0, bc=(PERIODIC, PERIODIC), **norm):
    return pixel_fields(x, u, v, dx, dy, bc, norm, torch.float64)[2]


def _absmax(t):
    """fmaxf over fabsf from 0: a NaN is skipped."""
    a = t.abs()
    a = torch.where(torch.isnan(a), torch.zeros_like(a), a)
    return a.amax((-2, -1))


def _finish(S, div, sqrt, P, Q, eps, N):
    """The nine sums by S and the finish by div / sqrt on tensors of the fields' dtype -> [B, T, 12]."""
    (UP, VP, wP, dP), (UQ, VQ, wQ, dQ) = P, Q
    KP, KQ = S(UP * UP + VP * VP), S(UQ * UQ + VQ * VQ)
    WP, WQ = S(wP * wP), S(wQ * wQ)
    DP, DQ = S(dP * dP), S(dQ * dQ)
    e = wP - wQ
    WE, WX = S(e * e), S(wP * wQ)
    a, b = UP - UQ, VP - VQ
    VE = S(a * a + b * b)
    half = torch.full_like(KP, 0.5)
    ke_P, ke_Q = div(half * KP, N), div(half * KQ, N)
    ens_P, ens_Q = div(half * WP, N), div(half * WQ, N)
    div_P, div_Q = sqrt(div(DP, N)), sqrt(div(DQ, N))
    vort_err = sqrt(div(WE, torch.where(WQ < eps, eps, WQ)))
    vort_cos = div(WX, (sqrt(WP) + eps) * (sqrt(WQ) + eps))
    vel_err = sqrt(div(VE, torch.where(KQ < eps, eps, KQ)))
    return torch.stack([ke_P, ke_Q, ens_P, ens_Q, div_P, div_Q, vort_err, vort_cos, vel_err, _absmax(wP), _absmax(wQ), _absmax(dP)], -1)


def _consts(y, dtype, norm):
    lead = y.shape[:2]
    H, W = y.shape[-2:]
    eps = _norm(y.shape[2], **norm)[6]
    N = torch.full(lead, float(H * W), dtype=dtype, device=y.device)
    epsv = torch.tensor(eps, dtype=torch.float32, device=y.device).to(dtype).expand(lead)
    return N, epsv


def statement32(y_hat, y, u=0, v=1, dx=1.0, dy=1.0, bc=(PERIODIC, PERIODIC), **norm):
    P, Q = pixel_fields(y_hat, u, v, dx, dy, bc, norm), pixel_fields(y, u, v, dx, dy, bc, norm)
    N, eps = _consts(y, torch.float32, norm)
    lead = y.shape[:2]

    def S(t):
        return sums32(t.reshape(lead + (-1,)))
    return _finish(S, _div32, _sqrt32, P, Q, eps, N)


def _own(y_hat, y, u, v, dx, dy, bc, norm, dtype):
    P, Q = pixel_fields(y_hat, u, v, dx, dy, bc, norm, dtype), pixel_fields(y, u, v, dx, dy, bc, norm, dtype)
    N, eps = _consts(y, dtype, norm)
    return _finish(lambda t: t.sum((-2, -1)), lambda a, b: a / b, torch.sqrt, P, Q, eps, N)


def stats64(y_hat, y, u=0, v=1, dx=1.0, dy=1.0, bc=(PERIODIC, PERIODIC), **norm):
    return _own(y_hat, y, u, v, dx, dy, bc, norm, torch.float64)


def stats32_torch(y_hat, y, u=0, v=1, dx=1.0, dy=1.0, bc=(PERIODIC, PERIODIC), **norm):
    return _own(y_hat, y, u, v, dx, dy, bc, norm, torch.float32)


def counts(y_hat, y, nbins, lo, hi, u=0, v=1, dx=1.0, dy=1.0, bc=(PERIODIC, PERIODIC), **norm):
    """-> int64 numpy [B, T, 2, nbins + 2]: the bin rule on the statement's fp32 vorticity of forecast (row 0) and truth (row 1)."""
    B, T = y.shape[:2]
    out = np.zeros((B, T, 2, nbins + 2), np.int64)
    for row, x in enumerate((y_hat, y)):
        k = bin_rule(vorticity32(x, u, v, dx, dy, bc, **norm).cpu().numpy(), lo, hi, nbins).reshape(B, T, -1)
        for i in range(B):
            for t in range(T):
                out[i, t, row] = np.bincount(k[i, t][k[i, t] >= 0], minlength=nbins + 2)
    return out

"""References of the field statistics (include/lns.h "field statistics"; lns_op_field_stats, lns_rollout_eval_stats), in
torch, on whatever device the inputs live on.

`statement32`: the statement of include/lns.h as explicit unfused fp32 ops in the written reduction order; the constants of
the denormalisation are device tensors, quotients and square roots are the correctly rounded ones.  The kernel is held to it
bit for bit.  `stats64`: every output in float64 from the same fp32 inputs (the denormalisation's constants rounded to fp32
first, as the lns_eval_spec holds them).  `stats32_torch`: the same quantities from torch's own fp32 reductions -- the `own`
of the project's rule max(2e-7, 3 x own).  `bin_rule` / `counts`: the histogram rule in numpy fp32.

Layouts: y_hat, y [B, T, C, H, W] -> [B, T, C, 12] in the order of NAMES.  `norm`: the keyword arguments of
lns_amd.engine.eval_spec."""
import numpy as np
import torch

from ensemble_score_reference import _div32, _norm, _sqrt32, denorm

NAMES = ("mean_P", "mean_Q", "var_P", "var_Q", "corr", "cos", "grad_y", "grad_x", "min_P", "max_P", "min_Q", "max_Q")

# the three families of the golden file (tools/make_golden_field_stats.py): statistics as in helpers.METRIC_STATS
GOLDEN_SEED = 23
GOLDEN = {
    "ns2d": dict(shape=(2, 3, 3, 13, 17), norm=dict(mean=0.37, std=1.9)),
    "sw": dict(shape=(2, 3, 3, 13, 17), norm=dict(mean=[0.4, -0.2, 9.5], std=[2.1, 1.7, 0.6])),
    # the two-phase denormalize() addresses channel 3 (VOF): four channels
    "twophase": dict(shape=(2, 3, 4, 13, 17), stats=(0.013, 0.21, 310.0, 180.0)),
}


def golden_norm(name):
    if name == "twophase":
        vm, vs, pm, ps = GOLDEN[name]["stats"]
        return dict(mean=[vm, vm, pm, 0.0], std=[vs, vs, ps, 1.0], zero_wall_channels=(0, 1), clamp_channels=(3,),
                    clamp=(0.0, 1.0 + 1e-8))
    return dict(GOLDEN[name]["norm"])


def golden_inputs(name):
    """Deterministic (torch-RNG-independent) pair: truth y ~ N(0,1), forecast y + 0.3 N(0,1); the two-phase VOF channel is
    spread over about (-0.5, 1.5) so that the clamp acts on both sides."""
    from lns_amd import filler
    shape = GOLDEN[name]["shape"]
    y = filler.normal("fs_y_" + name, shape, GOLDEN_SEED)
    yh = (y + 0.3 * filler.normal("fs_e_" + name, shape, GOLDEN_SEED)).astype(np.float32)
    if name == "twophase":
        y[:, :, 3] = 0.5 + 0.35 * y[:, :, 3]
        yh[:, :, 3] = 0.5 + 0.35 * yh[:, :, 3]
    return yh.astype(np.float32), y.astype(np.float32)


def sums32(x):
    """x [..., n] fp32 -> [...]: the statement's order.  Thread t of 256 adds terms t, t + 256, ... in ascending order
    starting from 0; the wave sum and the four-wave sum are a balanced binary tree over the 256 thread sums in thread order
    (every level adds neighbours; fp32 addition is commutative)."""
    lead, n = x.shape[:-1], x.shape[-1]
    pad = (-n) % 256
    if pad or n == 0:
        pad = pad if n else 256
        x = torch.cat([x, torch.zeros(lead + (pad,), dtype=x.dtype, device=x.device)], -1)
    rows = x.reshape(lead + (-1, 256))
    acc = torch.zeros(lead + (256,), dtype=x.dtype, device=x.device)
    for r in range(rows.shape[-2]):
        # a thread without a term in the last pass adds nothing (x + 0 = x, also for -0: the sum started from +0)
        acc = acc + rows[..., r, :]
    while acc.shape[-1] > 1:
        acc = acc[..., 0::2] + acc[..., 1::2]
    return acc[..., 0]


def _fd(v):
    """spatial_fd of the reference: central differences without wrap-around -> ([.., H-2, W], [.., H, W-2])."""
    return v[..., 2:, :] - v[..., :-2, :], v[..., :, 2:] - v[..., :, :-2]


def _skip_nan(v, fill):
    return torch.where(torch.isnan(v), torch.full_like(v, fill), v)


def statement32(y_hat, y, **norm):
    eps = _norm(y.shape[2], **norm)[6]
    P, Q = denorm(y_hat, norm), denorm(y, norm)
    H, W = P.shape[-2:]
    lead = P.shape[:3]

    def S(t):
        return sums32(t.reshape(lead + (-1,)))
    N = torch.full(lead, float(H * W), dtype=torch.float32, device=P.device)
    epsv = torch.full(lead, eps, dtype=torch.float32, device=P.device)
    zero = torch.zeros_like(N)
    SP, SQ, PP, QQ, PQ = S(P), S(Q), S(P * P), S(Q * Q), S(P * Q)
    mP, mQ = _div32(SP, N), _div32(SQ, N)
    cos = _div32(PQ, (_sqrt32(PP) + epsv) * (_sqrt32(QQ) + epsv))
    a, b = P - mP[..., None, None], Q - mQ[..., None, None]
    SA, SB, AA, BB, AB = S(a), S(b), S(a * a), S(b * b), S(a * b)
    vP = torch.fmax(_div32(AA - _div32(SA * SA, N), N), zero)
    vQ = torch.fmax(_div32(BB - _div32(SB * SB, N), N), zero)
    cov = _div32(AB - _div32(SA * SB, N), N)
    den = _sqrt32(vP) * _sqrt32(vQ)
    corr = torch.where(den == 0, zero, _div32(cov, torch.where(den == 0, torch.ones_like(den), den)))
    if H >= 3 and W >= 3:
        (gyP, gxP), (gyQ, gxQ) = _fd(P), _fd(Q)
        dy, dx = gyP - gyQ, gxP - gxQ
        GDy, GGy, GDx, GGx = S(dy * dy), S(gyQ * gyQ), S(dx * dx), S(gxQ * gxQ)
    else:
        GDy = GGy = GDx = GGx = zero
    gy = _sqrt32(_div32(GDy, torch.where(GGy < epsv, epsv, GGy)))
    gx = _sqrt32(_div32(GDx, torch.where(GGx < epsv, epsv, GGx)))
    inf = float("inf")
    ext = [_skip_nan(P, inf).amin((-2, -1)), _skip_nan(P, -inf).amax((-2, -1)),
           _skip_nan(Q, inf).amin((-2, -1)), _skip_nan(Q, -inf).amax((-2, -1))]
    return torch.stack([mP, mQ, vP, vQ, corr, cos, gy, gx] + ext, -1)


def _rest(P, Q, eps):
    """The statistics from denormalised fields with torch's own reductions, in the fields' dtype."""
    H, W = P.shape[-2:]
    d = (-2, -1)
    mP, mQ = P.mean(d), Q.mean(d)
    vP, vQ = P.var(d, unbiased=False), Q.var(d, unbiased=False)
    cov = ((P - mP[..., None, None]) * (Q - mQ[..., None, None])).mean(d)
    den = vP.sqrt() * vQ.sqrt()
    corr = torch.where(den == 0, torch.zeros_like(den), cov / torch.where(den == 0, torch.ones_like(den), den))
    cos = (P * Q).sum(d) / (((P * P).sum(d).sqrt() + eps) * ((Q * Q).sum(d).sqrt() + eps))
    if H >= 3 and W >= 3:
        (gyP, gxP), (gyQ, gxQ) = _fd(P), _fd(Q)
        e = torch.full_like(mP, eps)
        GGy, GGx = (gyQ * gyQ).sum(d), (gxQ * gxQ).sum(d)
        gy = (((gyP - gyQ) ** 2).sum(d) / torch.where(GGy < e, e, GGy)).sqrt()
        gx = (((gxP - gxQ) ** 2).sum(d) / torch.where(GGx < e, e, GGx)).sqrt()
    else:
        gy = gx = torch.zeros_like(mP)
    inf = float("inf")
    ext = [_skip_nan(P, inf).amin(d), _skip_nan(P, -inf).amax(d), _skip_nan(Q, inf).amin(d), _skip_nan(Q, -inf).amax(d)]
    return torch.stack([mP, mQ, vP, vQ, corr, cos, gy, gx] + ext, -1)


def denorm64_exact(x, norm):
    """D_c in float64 with the constants as Python floats (not rounded to fp32 first): what the reference's denormalize()
    computes on float64 tensors."""
    C, H, W = x.shape[-3:]
    mean, std, zero, clampc, lo, hi, _ = _norm(C, **norm)
    v = x.double() * torch.tensor(std, dtype=torch.float64).view(C, 1, 1) + torch.tensor(mean, dtype=torch.float64).view(C, 1, 1)
    for c in range(C):
        if zero[c]:
            v[..., c, 0, :] = 0.0
            v[..., c, -1, :] = 0.0
            v[..., c, :, 0] = 0.0
            v[..., c, :, -1] = 0.0
        if clampc[c]:
            v[..., c, :, :] = v[..., c, :, :].clamp(lo, hi)
    return v


def stats64(y_hat, y, exact_constants=False, **norm):
    eps = _norm(y.shape[2], **norm)[6]
    if exact_constants:
        return _rest(denorm64_exact(y_hat, norm), denorm64_exact(y, norm), eps)
    return _rest(denorm(y_hat, norm, torch.float64), denorm(y, norm, torch.float64), eps)


def stats32_torch(y_hat, y, **norm):
    eps = _norm(y.shape[2], **norm)[6]
    return _rest(denorm(y_hat, norm), denorm(y, norm), eps)


def bin_rule(v, lo, hi, nbins):
    """The bin of every value of the fp32 array v (include/lns.h): 0 below lo, nbins + 1 from hi on, else
    1 + min(nbins - 1, (int)((v - lo) * scale)) with scale = (float)nbins / (hi - lo), every op rounded to fp32; -1: a NaN."""
    v = np.asarray(v, np.float32)
    lo, hi = np.float32(lo), np.float32(hi)
    scale = np.float32(nbins) / np.float32(hi - lo)
    with np.errstate(invalid="ignore", over="ignore"):
        inner = np.nan_to_num(((v - lo).astype(np.float32) * scale).astype(np.float32), nan=0.0, posinf=0.0, neginf=0.0)
        k = 1 + np.minimum(nbins - 1, inner.astype(np.int64))
        out = np.where(v < lo, 0, np.where(v >= hi, nbins + 1, k))
    return np.where(np.isnan(v), -1, out).astype(np.int64)


def counts(y_hat, y, nbins, lo, hi, **norm):
    """-> int64 numpy [B, T, C, 2, nbins + 2]: the rule on the statement's fp32 fields (lo, hi: scalars or one per channel)."""
    C = y.shape[2]
    lo = [lo] * C if isinstance(lo, (int, float)) else list(lo)
    hi = [hi] * C if isinstance(hi, (int, float)) else list(hi)
    fields = [denorm(t, norm).cpu().numpy() for t in (y_hat, y)]
    B, T = y.shape[:2]
    out = np.zeros((B, T, C, 2, nbins + 2), np.int64)
    for row, f in enumerate(fields):
        for c in range(C):
            b = bin_rule(f[:, :, c], lo[c], hi[c], nbins).reshape(B, T, -1)
            for i in range(B):
                for t in range(T):
                    k = b[i, t]
                    out[i, t, c, row] = np.bincount(k[k >= 0], minlength=nbins + 2)
    return out


def emulate32(y_hat, y, **norm):
    """The statement on the CPU (strided thread sums, pairwise rest): statement32 on CPU tensors."""
    return statement32(y_hat.cpu(), y.cpu(), **norm)

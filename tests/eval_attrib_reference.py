"""References of the error attribution (include/lns.h "error attribution"; lns_op_eval_attrib, lns_rollout_eval_attrib), in
torch, on whatever device the inputs live on.

`statement32`: the statement as explicit unfused fp32 ops in the written reduction order (field_stats_reference.sums32); the
denominator G from the fp32 D_c(y), squared and summed in float64 in the same order and rounded once.  The kernels are held to
it bit for bit.
`statement64`: every column in float64 from the same fp32 inputs, RR and D included, so that the identity
frame^2 = prop^2 + recon^2 + cross can be checked.  `statement32_torch`: the same from torch's own fp32 reductions -- the
`own` of the project's rule max(2e-7, 3 x own).  `latent64`: the latent drift in float64.

Layouts: y_hat, r, y [B, T, C, H, W] -> dict of [B, T, C] (frame-wise) and [B, C] (sequence-wise) columns.  `norm`: the
keyword arguments of lns_amd.engine.eval_spec."""
import torch

from ensemble_score_reference import _div32, _norm, _sqrt32, denorm
from field_stats_reference import sums32

COLUMNS = ("prop_frame", "prop_seq", "cross_frame", "cross_seq")


def per_channel(norm):
    """engine.eval_spec's choice of the form: scalar mean and std and neither walls nor clamp -> the scalar form."""
    return (not isinstance(norm.get("mean", 0.0), (int, float))) or (not isinstance(norm.get("std", 1.0), (int, float))) or \
        len(norm.get("zero_wall_channels", ())) > 0 or len(norm.get("clamp_channels", ())) > 0


def differences(y_hat, r, y, norm, dtype=torch.float32, mistake=None):
    """-> (a, b, Q): the propagator's and the autoencoder's error and the denormalised truth, in `dtype`, each op rounded on its
    own.  Scalar form: the difference, then the scale; per-channel form: walls and clamp on all three operands first.
    mistake (the discrimination tests): "yhat_minus_y" forms a from (y_hat - y); "one_operand" denormalises r without walls and
    clamp in a."""
    if per_channel(norm):
        P, R, Q = denorm(y_hat, norm, dtype), denorm(r, norm, dtype), denorm(y, norm, dtype)
        Ra = R
        if mistake == "one_operand":
            plain = {k: v for k, v in norm.items() if k not in ("zero_wall_channels", "clamp_channels")}
            plain["mean"] = _norm(y.shape[2], **norm)[0]                # (stays per-channel)
            Ra = denorm(r, plain, dtype)
        a = P - (Q if mistake == "yhat_minus_y" else Ra)
        return a, R - Q, Q
    sd = torch.tensor(float(norm.get("std", 1.0)), dtype=torch.float32, device=y.device).to(dtype)
    mean = torch.tensor(float(norm.get("mean", 0.0)), dtype=torch.float32, device=y.device).to(dtype)
    yh, rr, yy = y_hat.to(dtype), r.to(dtype), y.to(dtype)
    a = (yh - (yy if mistake == "yhat_minus_y" else rr)) * sd
    return a, (rr - yy) * sd, yy * sd + mean


def _finish32(PP, XX, G, eps, half_cross=False):
    """[B, T, C] fp32 sums -> the four columns with the finish kernel's ops: t ascending running sums, correctly rounded / and sqrt."""
    epsv = torch.full_like(G, eps)
    two = torch.full_like(G, 1.0 if half_cross else 2.0)
    g = torch.where(G < epsv, epsv, G)
    out = dict(prop_frame=_sqrt32(_div32(PP, g)), cross_frame=_div32(two * XX, g))
    sp, sx, sg = (torch.zeros_like(PP[:, 0]) for _ in range(3))
    for t in range(PP.shape[1]):
        sp, sx, sg = sp + PP[:, t], sx + XX[:, t], sg + G[:, t]
    gs = torch.where(sg < epsv[:, 0], epsv[:, 0], sg)
    out.update(prop_seq=_sqrt32(_div32(sp, gs)), cross_seq=_div32(two[:, 0] * sx, gs))
    return out


def statement32(y_hat, r, y, **norm):
    """-> dict of COLUMNS (+ the sums PP, XX, G)."""
    eps = _norm(y.shape[2], **norm)[6]
    a, b, Q = differences(y_hat, r, y, norm)
    lead = y.shape[:3]
    PP, XX = sums32((a * a).reshape(lead + (-1,))), sums32((a * b).reshape(lead + (-1,)))
    Qd = Q.double()
    G = sums32((Qd * Qd).reshape(lead + (-1,))).float()
    out = _finish32(PP, XX, G, eps)
    out.update(PP=PP, XX=XX, G=G)
    return out


def _columns(PP, RR, XX, G, D, eps, denominator=None, half_cross=False):
    """The columns from sums of any dtype, with that dtype's ops (the float64 statement and torch's own fp32 version)."""
    def cols(PP, RR, XX, G, D, den):
        g = den.clamp_min(eps)
        k = 1.0 if half_cross else 2.0
        return dict(prop=(PP / g).sqrt(), recon=(RR / g).sqrt(), cross=k * XX / g, frame=(D / G.clamp_min(eps)).sqrt())
    f = cols(PP, RR, XX, G, D, G if denominator is None else denominator)
    s = cols(PP.sum(1), RR.sum(1), XX.sum(1), G.sum(1), D.sum(1), (G if denominator is None else denominator).sum(1))
    out = {k + "_frame": v for k, v in f.items()}
    out.update({k + "_seq": v for k, v in s.items()})
    return out


def _statement(y_hat, r, y, dtype, norm, mistake=None):
    eps = _norm(y.shape[2], **norm)[6]
    a, b, Q = differences(y_hat, r, y, norm, dtype, mistake if mistake in ("yhat_minus_y", "one_operand") else None)
    d = (-2, -1)
    den = None
    if mistake == "r_denominator":
        R = denorm(r, norm, dtype) if per_channel(norm) else b + Q
        den = (R * R).sum(d)
    return _columns((a * a).sum(d), (b * b).sum(d), (a * b).sum(d), (Q * Q).sum(d), ((a + b) * (a + b)).sum(d), eps, den,
                    half_cross=mistake == "half_cross")


def statement64(y_hat, r, y, mistake=None, **norm):
    """-> dict of prop / recon / cross / frame, _frame [B, T, C] and _seq [B, C], in float64.  mistake: one of the deliberate
    mistakes of the discrimination test ("r_denominator", "half_cross", "yhat_minus_y", "one_operand")."""
    return _statement(y_hat, r, y, torch.float64, norm, mistake)


def statement32_torch(y_hat, r, y, **norm):
    return _statement(y_hat, r, y, torch.float32, norm)


def latent64(z, z_true, eps=1e-8, own_norm=False):
    """z, z_true [B, T, ...] -> (latent_frame [B, T], latent_seq [B]) in float64; own_norm (a deliberate mistake): normalised
    by ||z_t||^2."""
    B, T = z.shape[:2]
    zz, zt = z.double().reshape(B, T, -1), z_true.double().reshape(B, T, -1)
    d2, g2 = ((zz - zt) ** 2).sum(-1), ((zz if own_norm else zt) ** 2).sum(-1)
    return (d2 / g2.clamp_min(eps)).sqrt(), (d2.sum(1) / g2.sum(1).clamp_min(eps)).sqrt()


def family(name, shape, g, gamma=0.5, alpha=0.2, beta=0.3):
    """The test inputs: truth y of the family (N(0,1), 1e-12 x, 1e12 x, 1e3 + 1e-2 x), r = y + alpha n1,
    y_hat = r + beta n2 + gamma (r - y) with noises of the truth's own fluctuation scale -- the gamma term makes cross more
    than a pure cancellation: 2 <a, b> = 2 gamma |b|^2 + noise.  -> (y_hat, r, y) fp32."""
    x = torch.randn(shape, generator=g, dtype=torch.float64)
    scale, off = {"unit": (1.0, 0.0), "tiny": (1e-12, 0.0), "huge": (1e12, 0.0), "offset": (1e-2, 1e3)}[name]
    y = off + scale * x
    n1 = scale * torch.randn(shape, generator=g, dtype=torch.float64)
    n2 = scale * torch.randn(shape, generator=g, dtype=torch.float64)
    r = y + alpha * n1
    yh = r + beta * n2 + gamma * (r - y)
    return yh.float(), r.float(), y.float()

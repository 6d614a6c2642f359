"""TEST INFRASTRUCTURE ONLY -- the tangent-linear rollout stated in plain torch on the CPU, in any dtype (float64: the ground
truth of tests/test_tangent_gpu.py).

  * `jvp_rollout` is torch.func.jvp over tests/train_reference.py's Propagator: forward-mode autograd of the very function
    the adjoint tests differentiate in reverse mode.  K tangents of a sample ride the batch axis (the samples of a batch do
    not interact: GroupNorm normalises per sample), row r = b*K + k;
  * `manual_jvp_rollout` is the same tangent written by hand the way the C code walks it (GroupNorm JVP, GELU', skip, scale,
    the row map), so that the deliberate mistakes of a hand-written JVP can be stated: VARIANTS.  Without a variant it is
    `jvp_rollout` to rounding (tests/test_tangent_cpu.py);
  * `mgs` is include/lns.h's statement of lns_op_orthonormalize in any dtype (float64: the truth; float32: every product,
    sum, projection and division in fp32, unfused -- the "fp32 statement" whose own error sets the tolerances);
  * `lyapunov` is the Benettin loop on `jvp_rollout` and `mgs`.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

import latent_fit_reference as lf
import train_reference as tr

VARIANTS = ("gn_drop_xhat_term", "gn_gamma_first", "gelu_at_output", "drop_skip", "cond_drop_scale", "row_map")
# the GPU grid: (engine, B, T, h, w) of the adjoint grid, and K tangents per sample
GRID = [(("E3", 2, 1, 4, 4), 1), (("E3", 4, 5, 8, 8), 3), (("E1", 3, 2, 3, 5), 2), (("E4", 1, 1, 3, 4), 4), (("E5", 1, 2, 2, 2), 5),
        (("E5", 3, 1, 1, 130), 2), (("E6", 5, 2, 7, 15), 3), (("E6", 33, 1, 2, 2), 2), (("E7", 3, 1, 7, 15), 1)]
DOT_GRID = [g for g in GRID if g[0][0] in ("E3", "E4", "E6")]
# (engine, B, T, h, w), K, renorm
LYAPUNOV = [(("E3", 2, 6, 4, 4), 4, 1), (("E3", 2, 6, 4, 4), 4, 2), (("E6", 2, 4, 7, 15), 3, 1), (("E5", 2, 4, 2, 2), 4, 1)]
ORTH_SHAPES = [(1, 1, 1), (2, 3, 32), (3, 4, 257), (2, 5, 1040), (1, 16, 4096), (2, 32, 32)]
V_SEED = 23


def grid_id(g):
    return "%s-K%d" % (tr.case_id(g[0]), g[1])


def applies(variant, case, K):
    """Whether the mistake changes anything at all on this case: the scale exists in the conditional block only, and the two
    row maps r // K and r % B differ only with B >= 2 and K >= 2 (the grid has them with B != K)."""
    name, B = case[0], case[1]
    if variant == "cond_drop_scale":
        return tr.ENGINES[name]["family"] == "twophase_cond"
    if variant == "row_map":
        return B >= 2 and K >= 2
    return True


def case_start(case, K):
    """(z0 [B,c,h,w], param [B] or None, v [B,K,c,h,w]): float32 numpy, a pure function of (case, K)."""
    from lns_amd import filler
    name, B, T, h, w = case
    _, z_in, _, prm = tr.case_inputs(case)
    v = filler.normal("tangent_v", (B, K, tr.ENGINES[name]["c"], h, w), V_SEED)
    return z_in[:, 0].copy(), prm, v


def _rows(t, K):
    return t.repeat_interleave(K, 0) if t is not None else None


def jvp_step(prop, z, param, vr, K):
    """(z_next [B,...], J v [B*K,...]) by forward-mode autograd; vr: [B*K,c,h,w]."""
    pr = _rows(param, K)
    zn, dv = torch.func.jvp(lambda q: prop(q, pr), (_rows(z, K),), (vr,))
    return zn[::K], dv


def jvp_rollout(prop, z0, param, v, T, step=jvp_step, **kw):
    """(z_pred [B,T,c,h,w], jv [B,K,T,c,h,w]) in z0's dtype."""
    B, K = v.shape[:2]
    z, vr, zs, js = z0, v.reshape((B * K,) + tuple(v.shape[2:])), [], []
    for _ in range(T):
        z, vr = step(prop, z, param, vr, K, **kw)
        zs.append(z)
        js.append(vr.reshape(v.shape))
    return torch.stack(zs, 1), torch.stack(js, 2)


# ---- the tangent by hand, where a hand-written JVP can go wrong ----------------------------------------------------------
def _conv_nb(prop, x, name, dil=1):
    """Propagator.conv without the bias: the tangent of a convolution."""
    w = prop.P[name + ".weight"]
    p = dil * (w.shape[-1] - 1) // 2
    if p:
        x = F.pad(x, (p, p, 0, 0), mode="circular" if prop.mode[1] == tr.CIRC else "constant")
        x = F.pad(x, (0, 0, p, p), mode="circular" if prop.mode[0] == tr.CIRC else "constant")
    return F.conv2d(x, w, None, dilation=dil)


def _gelu_grad(u):
    return 0.5 * (1.0 + torch.erf(u / math.sqrt(2.0))) + u * torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)


def _gn_jvp(prop, x, dx, name, idx, variant, groups=1, eps=1e-5):
    R, C = dx.shape[:2]
    xg = x.reshape(x.shape[0], groups, -1)
    mean, var = xg.mean(2, keepdim=True), xg.var(2, unbiased=False, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh, rs = ((xg - mean) * rstd)[idx], rstd[idx]
    g = prop.P[name + ".weight"].reshape(1, C, 1, 1)
    d = (dx * g if variant == "gn_gamma_first" else dx).reshape(R, groups, -1)
    proj = d - d.mean(2, keepdim=True)
    if variant != "gn_drop_xhat_term":
        proj = proj - xh * (d * xh).mean(2, keepdim=True)
    out = (rs * proj).reshape(dx.shape)
    return out if variant == "gn_gamma_first" else out * g


def manual_step(prop, z, param, vr, K, variant=None):
    assert variant is None or variant in VARIANTS, variant
    B, R = z.shape[0], vr.shape[0]
    r = torch.arange(R)
    idx = r % B if variant == "row_map" else r // K               # the tape's sample of tangent row r
    p = prop.pfx

    def dgelu(du, u):
        return du * _gelu_grad(F.gelu(u) if variant == "gelu_at_output" else u)[idx]
    x, dx = prop.conv(z, p + "in_proj"), _conv_nb(prop, vr, p + "in_proj")
    if prop.cond:
        ce = tr.fourier_embedding(param, prop.c, z.dtype)
        ce = prop.lin(F.gelu(prop.lin(ce, p + "cond_emb_proj.0")), p + "cond_emb_proj.2")
    for i in range(prop.nb):
        q = p + "net.%d" % i
        cv = ".conv1" if prop.cond else ".conv"
        u1 = prop.conv(prop.gn(x, q + cv + ".0"), q + cv + ".1")
        da1 = dgelu(_conv_nb(prop, _gn_jvp(prop, x, dx, q + cv + ".0", idx, variant), q + cv + ".1"), u1)
        if not prop.cond:
            u2 = prop.conv(F.gelu(u1), q + ".conv.3", prop.dil)
            da2 = dgelu(_conv_nb(prop, da1, q + ".conv.3", prop.dil), u2)
            x1 = x + prop.conv(F.gelu(u2), q + ".conv.5")
            dx1 = _conv_nb(prop, da2, q + ".conv.5") + (0 if variant == "drop_skip" else dx)
            xm, dxm = x1, dx1
        else:
            e = prop.lin(ce, q + ".cond_emb")[:, :, None, None]
            hh = prop.conv(F.gelu(u1), q + ".conv1.3", prop.dil) + e
            nc = prop.gn(hh, q + ".cond_conv1.0")
            dnc = _gn_jvp(prop, hh, _conv_nb(prop, da1, q + ".conv1.3", prop.dil), q + ".cond_conv1.0", idx, variant)
            x1 = x + prop.conv(F.gelu(nc), q + ".cond_conv1.2")
            dx1 = _conv_nb(prop, dgelu(dnc, nc), q + ".cond_conv1.2") + (0 if variant == "drop_skip" else dx)
            m = F.gelu(prop.conv(prop.gn(e, q + ".cond_conv2.0"), q + ".cond_conv2.1"))
            m = prop.conv(m, q + ".cond_conv2.3")
            xm = x1 * (1.0 + m)
            dxm = dx1 if variant == "cond_drop_scale" else dx1 * (1.0 + m)[idx]
        vv = prop.conv(prop.gn(xm, q + ".ffn.0"), q + ".ffn.1")
        dg = dgelu(_conv_nb(prop, _gn_jvp(prop, xm, dxm, q + ".ffn.0", idx, variant), q + ".ffn.1"), vv)
        x, dx = x1 + prop.conv(F.gelu(vv), q + ".ffn.3"), dx1 + _conv_nb(prop, dg, q + ".ffn.3")
    zn = prop.conv(prop.gn(x, p + "out_proj.0.gn", 32, 1e-6), p + "out_proj.1")
    return zn, _conv_nb(prop, _gn_jvp(prop, x, dx, p + "out_proj.0.gn", idx, variant, 32, 1e-6), p + "out_proj.1")


def manual_jvp_rollout(prop, z0, param, v, T, variant=None):
    return jvp_rollout(prop, z0, param, v, T, step=manual_step, variant=variant)


def case_run(case, K, dtype=torch.float64, variant=None, manual=False):
    """dict(z_pred [B,T,c,h,w], jv [B,K,T,c,h,w]) in numpy float64."""
    z0, prm, v = case_start(case, K)
    prop = lf.propagator(case[0], dtype)
    t = lambda a: torch.from_numpy(a).to(dtype) if a is not None else None      # noqa: E731
    with torch.no_grad():
        if manual or variant is not None:
            zp, jv = manual_jvp_rollout(prop, t(z0), t(prm), t(v), case[2], variant)
        else:
            zp, jv = jvp_rollout(prop, t(z0), t(prm), t(v), case[2])
    return dict(z_pred=zp.double().numpy(), jv=jv.double().numpy())


@functools.lru_cache(maxsize=None)
def truth(case, K):
    """(float64 run, float32 run): computed once per (case, K), shared, never modified."""
    return case_run(case, K), case_run(case, K, torch.float32)


# ---- orthonormalisation ---------------------------------------------------------------------------------------------------
def mgs(V, dtype=torch.float64):
    """include/lns.h's lns_op_orthonormalize on V [B,K,n], every operation in `dtype`: (Q [B,K,n], R [B,K,K], log R_kk
    [B,K]).  A zero remainder gives q = 0 and log R_kk = -inf."""
    Q = V.to(dtype).clone()
    B, K, _ = Q.shape
    R = torch.zeros((B, K, K), dtype=dtype)
    for k in range(K):
        for j in range(k):
            r = (Q[:, j] * Q[:, k]).sum(1)
            Q[:, k] = Q[:, k] - r[:, None] * Q[:, j]
            R[:, j, k] = r
        rkk = torch.sqrt((Q[:, k] * Q[:, k]).sum(1))
        R[:, k, k] = rkk
        Q[:, k] = torch.where(rkk[:, None] == 0, torch.zeros_like(Q[:, k]), Q[:, k] / rkk[:, None])
    return Q, R, torch.log(torch.diagonal(R, dim1=1, dim2=2))


def orth_input(shape, family="normal", seed=V_SEED):
    """float32 numpy [B,K,n]: N(0,1), or that times 1e-12 / 1e12."""
    from lns_amd import filler
    v = filler.normal("orth_v", tuple(shape), seed)
    return (v * np.float32({"normal": 1.0, "tiny": 1e-12, "huge": 1e12}[family])).astype(np.float32)


# ---- the Benettin loop ----------------------------------------------------------------------------------------------------
def lyapunov(prop, z0, param, V0, T, renorm=1, burn_in=0, dt=1.0):
    """(exponents [B,K], history [n_renorm,B,K], vectors [B,K,c,h,w], z_last) in z0's dtype: V0 [B,K,c,h,w] orthonormalised,
    carried by jvp_step, re-orthonormalised at the steps t with (T - t) % renorm == 0, log R_kk accumulated for t > burn_in."""
    dtype = z0.dtype
    B, K = V0.shape[:2]
    shape = V0.shape
    V = mgs(V0.reshape(B, K, -1), dtype)[0]
    logr, hist, z = torch.zeros((B, K), dtype=dtype), [], z0
    with torch.no_grad():
        for t in range(1, T + 1):
            z, vr = jvp_step(prop, z, param, V.reshape((B * K,) + tuple(shape[2:])), K)
            V = vr.reshape(B, K, -1)
            if (T - t) % renorm == 0:
                V, _, lr = mgs(V, dtype)
                if t > burn_in:
                    logr = logr + lr
                    hist.append(lr)
    return logr / ((T - burn_in) * dt), torch.stack(hist, 0), V.reshape(shape), z

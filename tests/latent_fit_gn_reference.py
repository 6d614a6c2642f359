"""TEST INFRASTRUCTURE ONLY -- the Gauss-Newton latent fit stated in plain torch / numpy on the CPU.

  * `gn_product` is include/lns.h's H v = sum_k (2 w_k / n) J_k^T (J_k v) + (2 lambda / n + mu) v through torch.func.jvp and
    torch.func.vjp of latent_fit_reference.rollout, in any dtype (float64: the truth; float32: the statement whose own error
    sets the tolerances), with v^T H v from the tangent side.  MISTAKES are four things a hand-written version gets wrong;
  * `gn_matrix` assembles H from an explicit Jacobian (torch.autograd.functional.jacobian), for shapes where n is small;
  * `block_sum`, `cg_start`, `cg_update` are the ORDER-EXACT float64 numpy statement of lns_op_cg_start / lns_op_cg_update:
    the same thread (i = tid, tid + 256, ... ascending), wave (butterfly, neighbours first) and block ((w0 + w1) + (w2 + w3))
    order, every element rounded to float32 once -- the GPU tests ask for equal bits;
  * `gn_fit` is the outer loop: n_cg steps of CG from delta = 0 on H delta = -g, then z0 += delta, no line search.
"""
import functools

import numpy as np
import torch

import latent_fit_reference as lf
import tangent_reference as tg
import train_reference as tr

MISTAKES = ("drop_weight", "step_off_by_one", "drop_diagonal", "beta_inverted")
OUTER, CG_ITERS = 3, 8
# What the float64 statement reaches on lf.TWINS (param known, observations lf.TWIN_STEPS / lf.TWIN_WEIGHTS, no damping, no
# background), worst sample of loss[0] / loss[-1]; tests/test_latent_fit_gn_cpu.py measures and asserts them with room (0.6 of
# the measured value), tests/test_latent_fit_gn_gpu.py asks the engine for half of the MEASURED value:
#                      E6 7x15     E6 2x2      E3 4x4
#   1 outer x 8 CG     17.5        9.2         17.2
#   3 outer x 8 CG     341         982         550
MEASURED = {(1, 8): {("E6", 3, 3, 7, 15): 17.5, ("E6", 3, 3, 2, 2): 9.2, ("E3", 3, 3, 4, 4): 17.2},
            (3, 8): {("E6", 3, 3, 7, 15): 341.0, ("E6", 3, 3, 2, 2): 982.0, ("E3", 3, 3, 4, 4): 550.0}}
CPU_FRACTION, GPU_FRACTION = 0.6, 0.5
# the grid of the GPU product tests: lf.ADJOINT_CASES, observations [0, T - 1] ([0] at T = 1), weights [1, 0.5]
GN_LAMBDA, GN_DAMPING = 0.3, 0.05
CG_SHAPES = [(B, n) for n in (1, 32, 257, 1040, 4096) for B in (1, 3)]


def case_obs(case):
    """(steps, weights) of a grid case."""
    T = case[2]
    return ([0, T - 1], [1.0, 0.5]) if T > 1 else ([0], [1.0])


def case_start(case):
    """(z0 [B,c,h,w], param [B] or None, v [B,c,h,w], u [B,c,h,w]): float32 numpy, a pure function of the case."""
    z0, prm, vu = tg.case_start(case, 2)
    return z0, prm, np.ascontiguousarray(vu[:, 0]), np.ascontiguousarray(vu[:, 1])


# ---- the product -----------------------------------------------------------------------------------------------------------
def gn_product(prop, z0, param, v, steps, weights=None, lam=0.0, mu=0.0, mistake=None):
    """(hv like v, vhv [B], jv [B, n_obs, ...]) in z0's dtype."""
    assert mistake is None or mistake in MISTAKES, mistake
    B = z0.shape[0]
    n = z0[0].numel()
    w = [1.0] * len(steps) if weights is None else list(weights)
    if mistake == "drop_weight":
        w = [1.0] * len(steps)
    T = steps[-1] + 1
    picked = [min(t + 1, T - 1) for t in steps] if mistake == "step_off_by_one" else list(steps)
    f = lambda z: lf.rollout(prop, z, param, T)        # noqa: E731
    _, jv = torch.func.jvp(f, (z0,), (v,))
    cot = torch.zeros_like(jv)
    vhv = torch.zeros(B, dtype=z0.dtype)
    for k, t in enumerate(picked):
        cot[:, t] = cot[:, t] + (2.0 * w[k] / n) * jv[:, t]
        vhv = vhv + (2.0 * w[k] / n) * (jv[:, t] ** 2).reshape(B, -1).sum(1)
    _, pull = torch.func.vjp(f, z0)
    hv, = pull(cot)
    cd = 0.0 if mistake == "drop_diagonal" else 2.0 * lam / n + mu
    hv = hv + cd * v
    vhv = vhv + cd * (v ** 2).reshape(B, -1).sum(1)
    return hv, vhv, jv[:, picked]


def gn_matrix(prop, z0, param, steps, weights=None, lam=0.0, mu=0.0):
    """H [B, n, n] from the explicit Jacobian of the rollout (the samples of a batch do not interact)."""
    B = z0.shape[0]
    n = z0[0].numel()
    w = [1.0] * len(steps) if weights is None else list(weights)
    T = steps[-1] + 1
    H = torch.zeros((B, n, n), dtype=z0.dtype)
    for b in range(B):
        pb = param[b:b + 1] if param is not None else None
        J = torch.autograd.functional.jacobian(lambda z: lf.rollout(prop, z, pb, T), z0[b:b + 1]).reshape(T, n, n)
        for k, t in enumerate(steps):
            H[b] += (2.0 * w[k] / n) * J[t].T @ J[t]
        H[b] += (2.0 * lam / n + mu) * torch.eye(n, dtype=z0.dtype)
    return H


@functools.lru_cache(maxsize=None)
def product_truth(case, lam, mu):
    """(float64 run, float32 run) of H v and H u on a grid case: dicts of numpy float64; computed once, shared."""
    z0, prm, v, u = case_start(case)
    steps, w = case_obs(case)
    out = []
    for dt in (torch.float64, torch.float32):
        prop = lf.propagator(case[0], dt)
        t = lambda a: torch.from_numpy(a).to(dt) if a is not None else None      # noqa: E731
        with torch.no_grad():
            hv, vhv, jv = gn_product(prop, t(z0), t(prm), t(v), steps, w, lam, mu)
            hu, uhu, ju = gn_product(prop, t(z0), t(prm), t(u), steps, w, lam, mu)
        out.append({k: a.double().numpy() for k, a in dict(hv=hv, vhv=vhv, jv=jv, hu=hu, uhu=uhu, ju=ju).items()})
    return tuple(out)


# ---- conjugate gradients, order-exact ----------------------------------------------------------------------------------------
def block_sum(terms):
    """The device's sum of float64 `terms` [n]: thread tid adds terms[tid], terms[tid + 256], ... ascending from 0.0, the 64
    lanes of a wave by the butterfly v = v + v[lane ^ m], m = 1, 2, .., 32, the four waves as (w0 + w1) + (w2 + w3)."""
    terms = np.asarray(terms, np.float64)
    n = terms.shape[0]
    rows = -(-n // 256)
    pad = np.zeros(rows * 256, np.float64)
    pad[:n] = terms
    acc = np.zeros(256, np.float64)
    for row in pad.reshape(rows, 256):
        acc = acc + row
    lanes = np.arange(256)
    for m in (1, 2, 4, 8, 16, 32):
        acc = acc + acc[lanes ^ m]
    return (acc[0] + acc[64]) + (acc[128] + acc[192])


def cg_start(g):
    """g [B, n] float32 -> (x, r, p float32 [B, n], rs, rs0 float64 [B])."""
    g = np.asarray(g, np.float32)
    r = -g
    rs = np.array([block_sum(r[b].astype(np.float64) ** 2) for b in range(g.shape[0])])
    return np.zeros_like(g), r.copy(), r.copy(), rs, rs.copy()


def cg_update(x, r, p, hp, rs, rs0, php=None, tol=0.0, applied=None, mistake=None):
    """One step, on copies: (x, r, p, rs, applied)."""
    x, r, p = (np.array(a, np.float32) for a in (x, r, p))
    hp = np.asarray(hp, np.float32)
    rs = np.array(rs, np.float64)
    applied = np.zeros(x.shape[0], np.int32) if applied is None else np.array(applied, np.int32)
    tol2 = np.float64(tol) * np.float64(tol)
    with np.errstate(all="ignore"):
        for b in range(x.shape[0]):
            d = np.float64(php[b]) if php is not None else block_sum(p[b].astype(np.float64) * hp[b].astype(np.float64))
            if not (np.isfinite(rs[b]) and rs[b] > 0 and np.isfinite(d) and d > 0 and rs[b] > tol2 * rs0[b]):
                continue
            alpha = rs[b] / d
            x[b] = (x[b].astype(np.float64) + alpha * p[b].astype(np.float64)).astype(np.float32)
            r[b] = (r[b].astype(np.float64) - alpha * hp[b].astype(np.float64)).astype(np.float32)
            rs_new = block_sum(r[b].astype(np.float64) ** 2)
            beta = rs[b] / rs_new if mistake == "beta_inverted" else rs_new / rs[b]
            p[b] = (r[b].astype(np.float64) + beta * p[b].astype(np.float64)).astype(np.float32)
            rs[b] = rs_new
            applied[b] += 1
    return x, r, p, rs, applied


def cg_solve(matvec, g, n_cg, dtype=torch.float64, mistake=None):
    """Plain CG in `dtype` on H delta = -g from 0, per sample: (delta, |r| / |r0| [B]).  matvec(p) -> (H p, p^T H p)."""
    B = g.shape[0]
    x, r = torch.zeros_like(g), -g
    p = r.clone()
    rs = (r * r).reshape(B, -1).sum(1)
    rs0 = rs.clone()
    shape = (B,) + (1,) * (g.dim() - 1)
    for _ in range(n_cg):
        hp, php = matvec(p)
        ok = (rs > 0) & (php > 0)
        alpha = torch.where(ok, rs / torch.where(ok, php, torch.ones_like(php)), torch.zeros_like(rs))
        x = x + alpha.reshape(shape) * p
        r = r - alpha.reshape(shape) * hp
        rs_new = torch.where(ok, (r * r).reshape(B, -1).sum(1), rs)
        safe = torch.where(ok, rs, torch.ones_like(rs))
        beta = torch.where(ok, safe / rs_new if mistake == "beta_inverted" else rs_new / safe, torch.zeros_like(rs))
        p = torch.where(ok.reshape(shape), r + beta.reshape(shape) * p, p)
        rs = rs_new
    return x, torch.sqrt(rs / rs0)


# ---- the outer loop ---------------------------------------------------------------------------------------------------------
def gn_fit(prop, z0, param, obs, steps, weights=None, outer=OUTER, n_cg=CG_ITERS, zb=None, lam=0.0, mu=0.0):
    """(z0, loss [outer + 1, B]): the loss before every outer iteration, then the loss of the returned state."""
    z = z0.detach().clone()
    losses = []
    for _ in range(outer):
        r = lf.fit_grads(prop, z, param, obs, steps, weights, zb, lam)
        losses.append(r["loss"])
        with torch.no_grad():
            delta, _ = cg_solve(lambda p: gn_product(prop, z, param, p, steps, weights, lam, mu)[:2], r["g_z"], n_cg, z.dtype)
        z = z + delta
    with torch.no_grad():
        losses.append(lf.obs_loss(lf.rollout(prop, z, param, steps[-1] + 1), obs, steps, weights, z, zb, lam)[0])
    return z, torch.stack(losses, 0)


def twin_fit(setup, dtype=torch.float64, outer=OUTER, n_cg=CG_ITERS, lam=0.0, mu=0.0):
    """gn_fit on a twin experiment of latent_fit_reference with `param` known: (z0, loss [outer + 1, B])."""
    d = lf.twin(setup)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype) if a is not None else None      # noqa: E731
    zb = t(d["z_start"]) if lam > 0 else None
    return gn_fit(lf.propagator(setup[0], dtype), t(d["z_start"]), t(d["p_true"]), t(d["obs"]), lf.TWIN_STEPS, lf.TWIN_WEIGHTS, outer,
                  n_cg, zb, lam, mu)

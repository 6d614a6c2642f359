"""TEST INFRASTRUCTURE ONLY -- the latent fit stated in plain torch on the CPU, in any dtype (float64: the ground truth).

  * the rollout is tests/train_reference.py's Propagator (itself written from the project's oracle and checked against the
    fixtures recorded from the real reference), with z0 and `param` as autograd leaves;
  * the observation loss is include/lns.h's definition, word for word:
        per[b, k] = mean_i (z_pred[b, t_k, i] - obs[b, k, i])^2
        loss[b]   = sum_k w_k per[b, k] + lambda mean_i (z0[b] - z_b[b])_i^2
    one loss per trajectory.  The samples of a batch do not interact (GroupNorm normalises per sample), so the gradient
    of sum_b loss[b] with respect to z0[b] / param[b] is the gradient of loss[b];
  * the fit loop is a hand-written Adam with torch.optim.Adam's formulas (no amsgrad, no weight decay);
  * `obs_grad_fp32` is a second, unfused float32 statement of lns_loss_obs_mse's two gradient outputs, op by op;
  * `grad_param_chain` opens the conditional path at ce (per block), at the two uses of emb and at fe, so that deliberate
    mistakes of a hand-written backward can be stated (tests/test_latent_fit_cpu.py: the inputs must tell them apart).
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

import train_reference as tr

ADJOINT_CASES = [("E3", 2, 1, 4, 4), ("E3", 4, 5, 8, 8), ("E1", 3, 2, 3, 5), ("E4", 1, 1, 3, 4), ("E5", 1, 2, 2, 2), ("E5", 3, 1, 1, 130),
                 ("E6", 5, 2, 7, 15), ("E6", 1, 1, 7, 15), ("E6", 33, 1, 2, 2), ("E7", 3, 1, 7, 15)]
COND_CASES = [c for c in ADJOINT_CASES if tr.ENGINES[c[0]]["family"] == "twophase_cond"]
# the twin experiments: engine, B, T, h, w; observations at steps [0, 2] with weights [1, 0.5]
TWINS = [("E6", 3, 3, 7, 15), ("E6", 3, 3, 2, 2), ("E3", 3, 3, 4, 4)]
TWIN_STEPS, TWIN_WEIGHTS = [0, 2], [1.0, 0.5]
TWIN_ITERS, LR_STATE, LR_PARAM = 40, 2e-3, 1e-2
STATE_NOISE, PARAM_OFFSET = 0.1, 0.2
# What the float64 statement reaches on TWINS after TWIN_ITERS iterations, worst sample (tests/test_latent_fit_cpu.py measures
# and asserts them with room; the GPU conditions of tests/test_latent_fit_gpu.py are at most half of the MEASURED factors):
#   loss[0] / loss[-1]:           7x15 6.9x, 2x2 5.8x, E3 4x4 6.8x                    -> CPU 4x, GPU 2x
#   param error, state and param: 7x15 0.2 -> 0.037 (5.4x); 2x2 0.2 -> 0.147 (1.36x: 64 observed numbers against 33
#                                 unknowns, one sample stays near its start)           -> CPU 4x / 1.2x, GPU 2x / 0.68x
#   param error, state known:     7x15 0.2 -> 0.0216 (9.2x), 2x2 0.2 -> 0.0202 (9.9x)  -> CPU 7x, GPU 4x
CPU_LOSS_RED, GPU_LOSS_RED = 4.0, 2.0
CPU_PARAM_RED = {("E6", 3, 3, 7, 15): 4.0, ("E6", 3, 3, 2, 2): 1.2}
GPU_PARAM_RED = {("E6", 3, 3, 7, 15): 2.0, ("E6", 3, 3, 2, 2): 0.68}
CPU_PARAM_ONLY_RED, GPU_PARAM_ONLY_RED = 7.0, 4.0
MISTAKES = ("swap_sin_cos", "drop_f", "dce_last_block", "drop_emb")


def propagator(name, dtype=torch.float64, cls=tr.Propagator, **kw):
    e = tr.ENGINES[name]
    from lns_amd import filler
    sd = filler.synthetic_state_dict(tr.prop_shapes(e["family"], e["c"], e["D"], e["blocks"]), tr.WEIGHT_SEED)
    P = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype) for k, v in sd.items()}
    return cls(P, e["family"], e["c"], e["D"], e["blocks"], e["dilation"], **kw)


def rollout(prop, z0, param, T):
    z, out = z0, []
    for _ in range(T):
        z = prop(z, param)
        out.append(z)
    return torch.stack(out, 1)


def obs_loss(z_pred, obs, steps, weights=None, z0=None, zb=None, lam=0.0):
    """(loss [B], per [B, n_obs]) in z_pred's dtype."""
    B = z_pred.shape[0]
    w = [1.0] * len(steps) if weights is None else list(weights)
    per = torch.stack([((z_pred[:, t] - obs[:, k]) ** 2).reshape(B, -1).mean(1) for k, t in enumerate(steps)], 1)
    loss = sum(w[k] * per[:, k] for k in range(len(steps)))
    if zb is not None:
        loss = loss + lam * ((z0 - zb) ** 2).reshape(B, -1).mean(1)
    return loss, per


def obs_grad_fp32(z_pred, obs, steps, weights=None, z0=None, zb=None, lam=0.0):
    """lns_loss_obs_mse's gradient outputs, unfused, in float32: (grad_z_pred, grad_z0_bg or None).  The coefficient is
    rounded once from double; a subtraction, then a multiplication."""
    assert z_pred.dtype == torch.float32 and obs.dtype == torch.float32
    n = z_pred[0, 0].numel()
    w = [1.0] * len(steps) if weights is None else list(weights)
    g = torch.zeros_like(z_pred)
    for k, t in enumerate(steps):
        coef = torch.tensor(np.float32(2.0 * w[k] / n))
        d = z_pred[:, t] - obs[:, k]
        g[:, t] = coef * d
    gbg = None
    if zb is not None:
        gbg = torch.tensor(np.float32(2.0 * lam / n)) * (z0 - zb)
    return g, gbg


def fit_grads(prop, z0, param, obs, steps, weights=None, zb=None, lam=0.0):
    """dict(loss [B], per, z_pred, g_z, g_p or None): loss and gradients of sum_b loss[b] at (z0, param)."""
    z = z0.detach().clone().requires_grad_(True)
    p = param.detach().clone().requires_grad_(True) if param is not None else None
    zp = rollout(prop, z, p, steps[-1] + 1)
    loss, per = obs_loss(zp, obs, steps, weights, z, zb, lam)
    loss.sum().backward()
    return dict(loss=loss.detach(), per=per.detach(), z_pred=zp.detach(), g_z=z.grad, g_p=p.grad if p is not None else None)


def adam(p, g, m, v, lr, step, betas=(0.9, 0.999), eps=1e-8):
    """torch.optim.Adam's single-tensor update, in place."""
    b1, b2 = betas
    m.mul_(b1).add_(g, alpha=1 - b1)
    v.mul_(b2).addcmul_(g, g, value=1 - b2)
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    denom = (v.sqrt() / math.sqrt(bc2)).add_(eps)
    p.addcdiv_(m, denom, value=-lr / bc1)


def fit(prop, z0, param, obs, steps, weights=None, iters=TWIN_ITERS, lr_state=LR_STATE, lr_param=LR_PARAM, fit_state=True,
        fit_param=True, zb=None, lam=0.0):
    """The fit loop -> (z0, param, loss [iters, B]) -- loss before each update."""
    z = z0.detach().clone()
    p = param.detach().clone() if param is not None else None
    fit_param = fit_param and p is not None
    mz, vz = torch.zeros_like(z), torch.zeros_like(z)
    mp, vp = (torch.zeros_like(p), torch.zeros_like(p)) if p is not None else (None, None)
    losses = []
    for it in range(iters):
        r = fit_grads(prop, z, p, obs, steps, weights, zb, lam)
        losses.append(r["loss"])
        if fit_state:
            adam(z, r["g_z"], mz, vz, lr_state, it + 1)
        if fit_param:
            adam(p, r["g_p"], mp, vp, lr_param, it + 1)
    return z, p, torch.stack(losses, 0)


@functools.lru_cache(maxsize=None)
def twin(setup):
    """A twin experiment's data, float32 numpy, a pure function of the setup: truth (z0, param), the observations of the
    float64 rollout of the truth (rounded to float32), and the perturbed start."""
    name, B, T, h, w = setup
    from lns_amd import filler
    e = tr.ENGINES[name]
    cond = e["family"] == "twophase_cond"
    z_true = filler.normal("twin_z", (B, e["c"], h, w), tr.INPUT_SEED) * np.float32(tr.Z_SCALE)
    p_true = filler.uniform01("twin_param", B, tr.INPUT_SEED).astype(np.float32) if cond else None
    prop = propagator(name)
    with torch.no_grad():
        zp = rollout(prop, torch.from_numpy(z_true).double(), torch.from_numpy(p_true).double() if cond else None, T)
    obs = zp[:, TWIN_STEPS].to(torch.float32).numpy()
    z_start = z_true + np.float32(STATE_NOISE) * filler.normal("twin_noise", z_true.shape, tr.INPUT_SEED)
    p_start = (p_true + np.float32(PARAM_OFFSET)) if cond else None
    return dict(z_true=z_true, p_true=p_true, obs=obs, z_start=z_start.astype(np.float32), p_start=p_start)


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double() if a is not None else None


# ---- the rollout adjoint on train_reference's case inputs: smooth-L1 against z_out, z0 and param as leaves -------------
def adjoint_reference(case, dtype=torch.float64):
    """dict(grad_z0 [B,c,h,w], grad_param [B] or None, z_pred), numpy float64."""
    name, B, T, h, w = case
    _, z_in, z_out, prm = tr.case_inputs(case)
    prop = propagator(name, dtype)
    z = torch.from_numpy(z_in[:, 0].copy()).to(dtype).requires_grad_(True)
    p = torch.from_numpy(prm).to(dtype).requires_grad_(True) if prm is not None else None
    zp = rollout(prop, z, p, T)
    F.smooth_l1_loss(zp, torch.from_numpy(z_out).to(dtype)).backward()
    f64 = lambda t: t.detach().to(torch.float64).numpy()      # noqa: E731
    return dict(grad_z0=f64(z.grad), grad_param=f64(p.grad) if p is not None else None, z_pred=f64(zp))


def rule(ours, ref64, ref32):
    """train_reference.bounds' rule for one tensor: (rel-L2 error, its bound, rel-max error, its bound, own rel-L2, own rel-max)."""
    o2, om = tr.rel_l2(ref32, ref64), tr.rel_max(ref32, ref64)
    return tr.rel_l2(ours, ref64), max(tr.GRAD_TOL, 3.0 * o2), tr.rel_max(ours, ref64), max(tr.GRAD_TOL, 3.0 * om), o2, om


@functools.lru_cache(maxsize=None)
def adjoint_truth(case):
    """(float64 run, float32 run): computed once per case, shared, never modified."""
    return adjoint_reference(case), adjoint_reference(case, torch.float32)


# ---- the chain down to param, opened where a hand-written backward can go wrong -----------------------------------------
class _OpenPropagator(tr.Propagator):
    drop_emb = False

    def cond_block(self, x, p, ce):
        e = self.lin(ce, p + ".cond_emb")[:, :, None, None]
        eh = e.detach() if self.drop_emb else e                 # the broadcast add into h
        h = F.gelu(self.conv(self.gn(x, p + ".conv1.0"), p + ".conv1.1"))
        h = self.conv(h, p + ".conv1.3", self.dil, dilated=True) + eh
        h = F.gelu(self.gn(h, p + ".cond_conv1.0"))
        x = x + self.conv(h, p + ".cond_conv1.2")
        m = F.gelu(self.conv(self.gn(e, p + ".cond_conv2.0"), p + ".cond_conv2.1"))
        m = self.conv(m, p + ".cond_conv2.3")
        h = F.gelu(self.conv(self.gn(x * (1.0 + m), p + ".ffn.0"), p + ".ffn.1"))
        return x + self.conv(h, p + ".ffn.3")

    def step(self, z, ces):
        p = self.pfx
        x = self.conv(z, p + "in_proj")
        for i in range(self.nb):
            x = self.cond_block(x, p + "net.%d" % i, ces[i])
        return self.conv(self.gn(x, p + "out_proj.0.gn", 32, 1e-6), p + "out_proj.1")


def grad_param_chain(case, mistake=None):
    """d loss / d param of adjoint_reference's problem in float64, by the chain the C code walks: d ce summed over the
    blocks (and the steps), d fe through cond_emb_proj, then the derivative of the Fourier embedding written out.
    mistake: None, or one of MISTAKES."""
    assert mistake is None or mistake in MISTAKES
    name, B, T, h, w = case
    _, z_in, z_out, prm = tr.case_inputs(case)
    prop = propagator(name, torch.float64, cls=_OpenPropagator)
    prop.drop_emb = mistake == "drop_emb"
    c = prop.c
    param = torch.from_numpy(prm).double()
    fe = tr.fourier_embedding(param, c, torch.float64).requires_grad_(True)
    ce = prop.lin(F.gelu(prop.lin(fe, prop.pfx + "cond_emb_proj.0")), prop.pfx + "cond_emb_proj.2")
    ces = [ce.detach().clone().requires_grad_(True) for _ in range(prop.nb)]
    z, preds = torch.from_numpy(z_in[:, 0].copy()).double(), []
    for _ in range(T):
        z = prop.step(z, ces)
        preds.append(z)
    F.smooth_l1_loss(torch.stack(preds, 1), torch.from_numpy(z_out).double()).backward()
    dce = ces[-1].grad if mistake == "dce_last_block" else sum(t.grad for t in ces)
    dfe, = torch.autograd.grad(ce, fe, dce)
    half = c // 2
    f = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float32) / half)          # float32 by definition
    a = (param.to(torch.float32)[:, None] * f[None]).double()
    f = f.double()
    if mistake == "drop_f":
        f = torch.ones_like(f)
    s, co = torch.sin(a), torch.cos(a)
    if mistake == "swap_sin_cos":
        s, co = co, s
    return (f[None] * (-s * dfe[:, :half] + co * dfe[:, half:2 * half])).sum(1).numpy()

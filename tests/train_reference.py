"""TEST INFRASTRUCTURE ONLY -- a plain torch.nn.functional statement of the stage-2 training rollout, differentiated by
autograd: the ground truth of the training gradients wherever no recorded fixture reaches.

Written from this project's own oracle (oracle/lns_oracle.py: OraclePropagator._block / _cond_block / forward,
fourier_embedding, teacher_forced_loss), not from the product: every convolution is F.pad + an unpadded F.conv2d, the
norms are F.group_norm, the loss is F.smooth_l1_loss.  It runs on the CPU in any dtype; in float64 it reproduces the four
fixtures recorded from the real reference (tests/golden/grads_*.npz) to the rounding of their storage
(tests/test_train_reference_cpu.py), which is what licenses it as the reference of tests/test_train_grad_shapes_gpu.py.

Also here, because three users share them (the CPU test, the GPU test, tools/train_grad_parity.py): the engines and
(B, T, h, w) cases of the shape grid, their deterministic inputs, and the two error measures.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

ZEROS, CIRC = 0, 1
PADDING = {                                     # family -> (mode_y, mode_x) of the propagator's "same" convolutions
    "ns2d": (CIRC, CIRC),
    "sw_half_periodic": (ZEROS, CIRC),
    "sw_nonsquared": (ZEROS, CIRC),
    "twophase": (ZEROS, ZEROS),
    "twophase_cond": (ZEROS, ZEROS),
}
# deliberate mistakes (tests/test_train_reference_cpu.py: the grid's inputs must tell each of them from the truth)
VARIANTS = ("dilation", "pad_x", "mirror", "bt_mixup")


def prop_shapes(family, c, D, n_block, prefix="propagator."):
    """{state_dict key: shape} of the propagator (E = c: LatentDynamics builds the conditional one with cond_emb_dim =
    latent_dim), in the order of the engine's parameter table."""
    cond = family == "twophase_cond"
    s = {}

    def conv(name, co, ci, k, bias=True):
        s[name + ".weight"] = (co, ci, k, k)
        if bias:
            s[name + ".bias"] = (co,)

    def norm(name):
        s[name + ".weight"] = (D,)
        s[name + ".bias"] = (D,)

    def lin(name, o, i):
        s[name + ".weight"] = (o, i)
        s[name + ".bias"] = (o,)
    conv(prefix + "in_proj", D, c, 1)
    if cond:
        lin(prefix + "cond_emb_proj.0", c, c)
        lin(prefix + "cond_emb_proj.2", c, c)
    for i in range(n_block):
        p = prefix + "net.%d" % i
        if cond:
            lin(p + ".cond_emb", D, c)
            norm(p + ".conv1.0"); conv(p + ".conv1.1", D, D, 3); conv(p + ".conv1.3", D, D, 3)
            norm(p + ".cond_conv1.0"); conv(p + ".cond_conv1.2", D, D, 3)
            norm(p + ".cond_conv2.0"); conv(p + ".cond_conv2.1", D, D, 1); conv(p + ".cond_conv2.3", D, D, 1)
        else:
            norm(p + ".conv.0"); conv(p + ".conv.1", D, D, 3); conv(p + ".conv.3", D, D, 3); conv(p + ".conv.5", D, D, 3)
        norm(p + ".ffn.0"); conv(p + ".ffn.1", D, D, 1, bias=False); conv(p + ".ffn.3", D, D, 1, bias=False)
    norm(prefix + "out_proj.0.gn")
    conv(prefix + "out_proj.1", c, D, 1)
    return s


def fourier_embedding(t, dim, dtype, max_period=10000):
    """oracle fourier_embedding: float32 by definition (frequencies, argument, cos / sin), then cast to the run's dtype."""
    half = dim // 2
    freqs = torch.exp(-math.log(max_period) * torch.arange(half, dtype=torch.float32) / half)
    a = t.to(torch.float32)[:, None] * freqs[None]
    emb = torch.cat([torch.cos(a), torch.sin(a)], dim=-1)
    if dim % 2:
        emb = torch.cat([emb, torch.zeros_like(emb[:, :1])], dim=-1)
    return emb.to(dtype)


class Propagator:
    """The propagator as a function of a {key: tensor} dict.  variant: None, or one of VARIANTS (a deliberate mistake)."""

    def __init__(self, P, family, c, D, n_block, dilation, prefix="propagator.", variant=None):
        assert variant is None or variant in VARIANTS, variant
        self.P, self.pfx, self.c, self.D, self.nb = P, prefix, c, D, n_block
        self.cond = family == "twophase_cond"
        my, mx = PADDING[family]
        self.dil = dilation
        if variant == "dilation":                          # off by one: down where there is room, up at dilation 1
            self.dil = dilation - 1 if dilation > 1 else dilation + 1
        if variant == "pad_x":
            mx = ZEROS if mx == CIRC else CIRC
        self.mode = (my, mx)
        self.mirror = variant == "mirror"

    def conv(self, x, name, dil=1, dilated=False):
        w, b = self.P[name + ".weight"], self.P.get(name + ".bias")
        if dilated and self.mirror:
            w = w.flip(2, 3)
        p = dil * (w.shape[-1] - 1) // 2
        if p:
            x = F.pad(x, (p, p, 0, 0), mode="circular" if self.mode[1] == CIRC else "constant")
            x = F.pad(x, (0, 0, p, p), mode="circular" if self.mode[0] == CIRC else "constant")
        return F.conv2d(x, w, b, dilation=dil)

    def gn(self, x, name, groups=1, eps=1e-5):
        return F.group_norm(x, groups, self.P[name + ".weight"], self.P[name + ".bias"], eps)

    def lin(self, x, name):
        return F.linear(x, self.P[name + ".weight"], self.P[name + ".bias"])

    def block(self, x, p):
        h = self.gn(x, p + ".conv.0")
        h = F.gelu(self.conv(h, p + ".conv.1"))
        h = F.gelu(self.conv(h, p + ".conv.3", self.dil, dilated=True))
        x = x + self.conv(h, p + ".conv.5")
        h = F.gelu(self.conv(self.gn(x, p + ".ffn.0"), p + ".ffn.1"))
        return x + self.conv(h, p + ".ffn.3")

    def cond_block(self, x, p, ce):
        e = self.lin(ce, p + ".cond_emb")[:, :, None, None]
        h = F.gelu(self.conv(self.gn(x, p + ".conv1.0"), p + ".conv1.1"))
        h = self.conv(h, p + ".conv1.3", self.dil, dilated=True) + e
        h = F.gelu(self.gn(h, p + ".cond_conv1.0"))
        x = x + self.conv(h, p + ".cond_conv1.2")
        m = F.gelu(self.conv(self.gn(e, p + ".cond_conv2.0"), p + ".cond_conv2.1"))
        m = self.conv(m, p + ".cond_conv2.3")
        h = F.gelu(self.conv(self.gn(x * (1.0 + m), p + ".ffn.0"), p + ".ffn.1"))
        return x + self.conv(h, p + ".ffn.3")

    def __call__(self, z, param=None):
        p = self.pfx
        x = self.conv(z, p + "in_proj")
        if self.cond:
            ce = fourier_embedding(param, self.c, z.dtype)
            ce = self.lin(F.gelu(self.lin(ce, p + "cond_emb_proj.0")), p + "cond_emb_proj.2")
            for i in range(self.nb):
                x = self.cond_block(x, p + "net.%d" % i, ce)
        else:
            for i in range(self.nb):
                x = self.block(x, p + "net.%d" % i)
        return self.conv(self.gn(x, p + "out_proj.0.gn", 32, 1e-6), p + "out_proj.1")


def training_rollout(sd, family, c, D, n_block, dilation, z_in, z_out, param=None, dtype=torch.float64, prefix="propagator.",
                     variant=None, loss_fn=F.smooth_l1_loss):
    """LatentDynamics.forward(z_in, z_out[, param], loss_fn) + loss.backward() on the CPU in `dtype`.
    sd: {key: ndarray} holding (at least) the propagator's entries; z_in [B,1,c,h,w], z_out [B,T,c,h,w], param [B] or None.
    Returns dict(loss, z_pred [B,T,c,h,w], grads {key: array}, grad_z_in [B,1,c,h,w]), all numpy float64."""
    keys = list(prop_shapes(family, c, D, n_block, prefix))
    P = {k: torch.from_numpy(np.ascontiguousarray(sd[k])).to(dtype).requires_grad_(True) for k in keys}
    for k, shp in prop_shapes(family, c, D, n_block, prefix).items():
        assert tuple(P[k].shape) == shp, (k, tuple(P[k].shape), shp)
    zi = torch.from_numpy(np.ascontiguousarray(z_in)).to(dtype).requires_grad_(True)
    zo = torch.from_numpy(np.ascontiguousarray(z_out)).to(dtype)
    pt = torch.from_numpy(np.ascontiguousarray(param)).to(dtype) if param is not None else None
    prop = Propagator(P, family, c, D, n_block, dilation, prefix, variant)
    B, T = zo.shape[:2]
    z, preds = zi[:, 0], []
    for _ in range(T):
        z = prop(z, pt)
        preds.append(z)
    z_pred = torch.stack(preds, 1)
    scored = z_pred
    if variant == "bt_mixup":                              # the [B][T] tensor read as if it were [T][B]
        scored = z_pred.reshape((T, B) + tuple(z_pred.shape[2:])).transpose(0, 1)
    loss = loss_fn(scored, zo)
    loss.backward()
    f64 = lambda t: t.detach().to(torch.float64).numpy()      # noqa: E731
    return dict(loss=np.float64(loss.item()), z_pred=f64(z_pred), grads={k: f64(P[k].grad) for k in keys}, grad_z_in=f64(zi.grad))


# ---- the shape grid ------------------------------------------------------------------------------------------------
# name -> family, (c, D, blocks, dilation), and the smallest model lns_create accepts around that propagator: a preset of
# lns_amd.config with overrides (the autoencoder only has to exist; the training calls take h and w as arguments).
_SW_MINI = dict(Ly=24, Lx=48, resolutions=[24, 48], in_channels=3, latent_resolution=6, encoder_channels=[32, 32, 64, 64],
                decoder_channels=[64, 32, 32], attn_resolutions=[12], decoder_attn_heads=2, decoder_attn_dim=32)
ENGINES = {
    "E1": dict(family="ns2d", c=16, D=128, blocks=3, dilation=2, preset="ns2d_mini", overrides={}),
    "E2": dict(family="ns2d", c=8, D=96, blocks=1, dilation=3, preset="ns2d_mini", overrides={}),
    "E3": dict(family="ns2d", c=8, D=32, blocks=2, dilation=1, preset="ns2d_mini", overrides={}),
    "E4": dict(family="sw_half_periodic", c=64, D=128, blocks=4, dilation=3, preset="sw_half_periodic", overrides=_SW_MINI),
    "E5": dict(family="twophase", c=8, D=64, blocks=2, dilation=2, preset="cond_ae_mini", overrides=dict(cond_encoder=False)),
    "E6": dict(family="twophase_cond", c=8, D=64, blocks=2, dilation=2, preset="cond_ae_mini",
               overrides=dict(cond_encoder=False, family="twophase_cond")),
    "E7": dict(family="twophase_cond", c=64, D=128, blocks=4, dilation=2, preset="cond_ae_mini",
               overrides=dict(cond_encoder=False, family="twophase_cond")),
}
CASES = [
    ("E1", 33, 1, 8, 8), ("E1", 5, 2, 16, 16), ("E1", 1, 3, 8, 8), ("E1", 3, 2, 3, 5),
    ("E2", 3, 2, 5, 13), ("E2", 1, 1, 7, 9),
    ("E3", 4, 5, 8, 8), ("E3", 2, 1, 4, 4),
    ("E4", 3, 2, 12, 24), ("E4", 1, 1, 3, 4),
    ("E5", 5, 2, 7, 15), ("E5", 3, 1, 1, 130), ("E5", 1, 2, 2, 2),
    ("E6", 5, 2, 7, 15), ("E6", 300, 1, 2, 2), ("E6", 1, 1, 7, 15),
    ("E7", 3, 1, 7, 15),
]
WEIGHT_SEED, INPUT_SEED, Z_SCALE = 3, 11, 0.5
GRAD_TOL = 1e-4            # tests/test_gpu_parity.py


def case_id(case):
    return "%s-B%d-T%d-%dx%d" % case


def engine_args(name):
    """The `args` namespace of the drop-in model that carries engine `name`'s propagator."""
    from lns_amd import config
    e = ENGINES[name]
    over = dict(e["overrides"], latent_dim=e["c"], prop_n_embd=e["D"], prop_n_block=e["blocks"], dilation=e["dilation"])
    return config.preset(e["preset"], **over)


def case_inputs(case):
    """(propagator state dict, z_in [B,1,c,h,w], z_out [B,T,c,h,w], param [B] or None): float32, a pure function of the case."""
    from lns_amd import filler
    name, B, T, h, w = case
    e = ENGINES[name]
    sd = filler.synthetic_state_dict(prop_shapes(e["family"], e["c"], e["D"], e["blocks"]), WEIGHT_SEED)
    z_in = filler.normal("z_in", (B, 1, e["c"], h, w), INPUT_SEED) * np.float32(Z_SCALE)
    z_out = filler.normal("z_out", (B, T, e["c"], h, w), INPUT_SEED) * np.float32(Z_SCALE)
    prm = filler.uniform01("param", B, INPUT_SEED).astype(np.float32) if e["family"] == "twophase_cond" else None
    return sd, z_in, z_out, prm


def case_reference(case, dtype=torch.float64, variant=None):
    e = ENGINES[case[0]]
    sd, z_in, z_out, prm = case_inputs(case)
    return training_rollout(sd, e["family"], e["c"], e["D"], e["blocks"], e["dilation"], z_in, z_out, prm, dtype=dtype, variant=variant)


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).sum() / (b ** 2).sum()))


def rel_max(a, b):
    """max |a - b| / max |b|: one wrong element comparable to the largest shows, however large the tensor."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def tensors_of(r):
    """{name: array} of everything a run is judged on tensor by tensor: every parameter gradient and grad_z_in."""
    t = dict(r["grads"])
    t["grad_z_in"] = r["grad_z_in"]
    return t


def bounds(ref64, ref32):
    """{name: (rel-L2 bound, rel-max bound, own rel-L2, own rel-max)}: max(GRAD_TOL, 3 x own), `own` being the float32 CPU
    run of this same reference against its float64 run, in the measure the bound is applied to."""
    out = {}
    t64, t32 = tensors_of(ref64), tensors_of(ref32)
    for k in t64:
        o2, om = rel_l2(t32[k], t64[k]), rel_max(t32[k], t64[k])
        out[k] = (max(GRAD_TOL, 3.0 * o2), max(GRAD_TOL, 3.0 * om), o2, om)
    return out


# ---- the GPU side of the grid (tests/test_train_grad_shapes_gpu.py, tools/train_grad_parity.py) ------------------------
FORMS = [0, 1]             # option "train_wgrad": one block per output tile / batch-parallel


@functools.lru_cache(maxsize=None)
def grid_model(name):
    """The drop-in model around engine `name`'s propagator, built as gpu_checks.build_models does, autoencoder frozen."""
    import gpu_checks as gc
    model, _ = gc.build_models(engine_args(name), WEIGHT_SEED)
    for p_ in model._ae.parameters():
        p_.requires_grad_(False)
    return model


@functools.lru_cache(maxsize=None)
def truth(case):
    """(float64 reference, per-tensor bounds): computed once per case, shared by both forms, never modified."""
    r64 = case_reference(case)
    return r64, bounds(r64, case_reference(case, dtype=torch.float32))


def engine_run(case, form):
    """model(z_in, z_out, *tail) + backward() on the HIP engine -> the dict training_rollout returns."""
    name, B, T, h, w = case
    model = grid_model(name)
    model._owner._eng.set_option("train_wgrad", form)
    _, z_in, z_out, prm = case_inputs(case)
    zi = torch.from_numpy(z_in).cuda().requires_grad_(True)
    zo = torch.from_numpy(z_out).cuda()
    seen = {}

    def loss_fn(pred, target):
        seen["z_pred"] = pred.detach()
        return F.smooth_l1_loss(pred, target)
    tail = (torch.from_numpy(prm).cuda(), loss_fn) if prm is not None else (loss_fn,)
    params = {k: p_ for k, p_ in model.named_parameters() if k.startswith("propagator.")}
    for p_ in params.values():
        p_.grad = None
    loss = model(zi, zo, *tail)
    loss.backward()
    torch.cuda.synchronize()
    assert all(p_.grad is None for p_ in model._ae.parameters())
    return dict(loss=np.float64(loss.item()), z_pred=seen["z_pred"].cpu().numpy().astype(np.float64),
                grads={k: p_.grad.detach().cpu().numpy().astype(np.float64) for k, p_ in params.items()},
                grad_z_in=zi.grad.cpu().numpy().astype(np.float64))


def compare(case, form):
    """[(tensor, rel-L2 error, its bound, rel-max error, its bound, own rel-L2, own rel-max)] and the loss / z_pred errors."""
    r64, bnd = truth(case)
    got = engine_run(case, form)
    assert list(got["grads"]) == list(r64["grads"])
    rows = []
    t64, tg = tensors_of(r64), tensors_of(got)
    for k in t64:
        assert tg[k].shape == t64[k].shape and np.isfinite(tg[k]).all(), k
        b2, bm, o2, om = bnd[k]
        rows.append((k, rel_l2(tg[k], t64[k]), b2, rel_max(tg[k], t64[k]), bm, o2, om))
    return rows, abs(got["loss"] - r64["loss"]), r64["loss"], rel_l2(got["z_pred"], r64["z_pred"])

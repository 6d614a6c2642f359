"""Python owner of an `lns_engine` handle (include/lns.h).

Translates the reference's `args` namespace into `lns_config`, exposes the
engine's parameter table (= the reference state_dict keys/shapes) and runs the
hot path on CUDA/HIP tensors.  torch is used for device memory and streams only.
"""
import collections
import contextlib
import ctypes
import functools
import numbers
import types

import numpy as np

from . import _lib
from ._lib import (LNS_AE_HALF_PERIODIC, LNS_AE_NONE, LNS_AE_NONSQUARED, LNS_AE_SQUARE,
                   LNS_PAD_CIRCULAR, LNS_PAD_ZEROS, LNS_PROP_CONDITIONAL, LNS_PROP_NONE,
                   LNS_PROP_PLAIN, LnsConfig, LnsError)

# family -> (ae kind, propagator kind)
_FAMILIES = {
    "ns2d": (LNS_AE_SQUARE, LNS_PROP_PLAIN),
    "sw_half_periodic": (LNS_AE_HALF_PERIODIC, LNS_PROP_PLAIN),
    "sw_nonsquared": (LNS_AE_NONSQUARED, LNS_PROP_PLAIN),
    "twophase": (LNS_AE_NONSQUARED, LNS_PROP_PLAIN),
    "twophase_cond": (LNS_AE_NONSQUARED, LNS_PROP_CONDITIONAL),
}


def _fill_list(cfg, name, values):
    values = list(values or [])
    if len(values) > _lib.LNS_MAX_STAGES:
        raise ValueError("%s: at most %d entries" % (name, _lib.LNS_MAX_STAGES))
    arr = getattr(cfg, name)
    for i, v in enumerate(values):
        arr[i] = int(v)
    setattr(cfg, "n_" + name, len(values))


def make_config(args, ae_kind=None, prop_kind=None, ae_prefix="", prop_prefix="",
                prop_pad=None) -> LnsConfig:
    """`args` carries the reference's YAML keys (modules/autoencoder2d.py:19-27,78-92;
    train_stage2_ns2d.py:94-104).  `family` (optional) selects the AE / propagator files."""
    fam = getattr(args, "family", None)
    if ae_kind is None or prop_kind is None:
        if fam not in _FAMILIES:
            raise ValueError("args.family must be one of %s" % sorted(_FAMILIES))
        ak, pk = _FAMILIES[fam]
        ae_kind = ak if ae_kind is None else ae_kind
        prop_kind = pk if prop_kind is None else prop_kind
    c = LnsConfig()
    c.abi_version = _lib.LNS_ABI_VERSION
    c.ae_kind, c.prop_kind = ae_kind, prop_kind
    c.latent_dim = int(args.latent_dim)
    if ae_kind != LNS_AE_NONE:
        c.in_channels = int(args.in_channels)
        c.Ly, c.Lx = int(args.Ly), int(args.Lx)
        if ae_kind == LNS_AE_SQUARE:
            c.res_h = c.res_w = int(args.resolution)
            heads, dim = args.attn_heads, args.attn_dim
            per = bool(args.is_periodic)
            c.ae_pad_y = c.ae_pad_x = LNS_PAD_CIRCULAR if per else LNS_PAD_ZEROS
            c.use_attn_enc = int(bool(getattr(args, "use_attn_enc", False)))
        else:
            c.res_h, c.res_w = int(args.resolutions[0]), int(args.resolutions[1])
            heads, dim = args.decoder_attn_heads, args.decoder_attn_dim
            c.hw_ratio = float(getattr(args, "hw_ratio", c.res_w / c.res_h))
            if ae_kind == LNS_AE_HALF_PERIODIC:
                pd = args.periodic_direction
                if pd not in ("x", "y"):
                    raise ValueError("periodic_direction must be x or y")
                c.ae_pad_y = LNS_PAD_CIRCULAR if pd == "y" else LNS_PAD_ZEROS
                c.ae_pad_x = LNS_PAD_CIRCULAR if pd == "x" else LNS_PAD_ZEROS
            else:
                per = bool(args.is_periodic)
                c.ae_pad_y = c.ae_pad_x = LNS_PAD_CIRCULAR if per else LNS_PAD_ZEROS
        c.latent_resolution = int(args.latent_resolution)
        _fill_list(c, "encoder_channels", args.encoder_channels)
        _fill_list(c, "decoder_channels", args.decoder_channels)
        _fill_list(c, "attn_resolutions", args.attn_resolutions)
        _fill_list(c, "fourier_resolutions", getattr(args, "fourier_resolutions", []))
        c.encoder_res_blocks = int(args.encoder_res_blocks)
        c.decoder_res_blocks = int(args.decoder_res_blocks)
        c.use_fa = int(bool(args.use_fa))
        c.final_smoothing = int(bool(args.final_smoothing))
        dca = getattr(args, "disable_coarse_attn", None)
        c.disable_coarse_attn = int(bool(dca)) if dca is not None else 0
        c.attn_heads, c.attn_dim = int(heads), int(dim)
    if prop_kind != LNS_PROP_NONE:
        c.prop_n_block = int(args.prop_n_block)
        c.prop_n_embd = int(args.prop_n_embd)
        c.prop_dilation = int(args.dilation)
        if prop_pad is None:
            # train_stage2_ns2d.py:75 circular; train_stage2_SW.py:76 periodic_direction='x';
            # train_stage2_twophase.py:76 / _conditional.py:106 zeros
            prop_pad = {"ns2d": (LNS_PAD_CIRCULAR, LNS_PAD_CIRCULAR),
                        "sw_half_periodic": (LNS_PAD_ZEROS, LNS_PAD_CIRCULAR),
                        "sw_nonsquared": (LNS_PAD_ZEROS, LNS_PAD_CIRCULAR)}.get(
                            fam, (LNS_PAD_ZEROS, LNS_PAD_ZEROS))
        c.prop_pad_y, c.prop_pad_x = prop_pad
        c.cond_emb_dim = int(getattr(args, "cond_emb_dim", args.latent_dim))
    if getattr(args, "cond_encoder", False):
        # ConditionalSimpleAutoencoder (modules/autoencoder2d_nonsquared.py:279-305): CondEncoder + plain Decoder
        if ae_kind != LNS_AE_NONSQUARED:
            raise ValueError("cond_encoder is defined for the non-squared autoencoder only")
        c.cond_encoder = 1
        c.cond_emb_channels = int(args.cond_emb_channels)
    c.ae_prefix = ae_prefix.encode()
    c.prop_prefix = prop_prefix.encode()
    return c


def adam_spec(lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, step=1):
    """`lns_adam_spec` from torch.optim.Adam's hyper-parameters; `step` is the 1-based count of the update."""
    spec = _lib.LnsAdamSpec()
    spec.size = ctypes.sizeof(_lib.LnsAdamSpec)
    spec.lr, spec.beta1, spec.beta2 = float(lr), float(betas[0]), float(betas[1])
    spec.eps, spec.weight_decay, spec.step = float(eps), float(weight_decay), int(step)
    return spec


def update_spec(lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, step=1, max_norm=0.0, decoupled=False, skip_nonfinite=False):
    """`lns_update_spec`: adam_spec's fields, the clip threshold (`max_norm` <= 0 or None: the norm is computed, nothing is
    clipped) and the LNS_UPDATE_* flags (decoupled: AdamW's weight decay; skip_nonfinite: no update on an inf / NaN norm)."""
    spec = _lib.LnsUpdateSpec()
    spec.size = ctypes.sizeof(_lib.LnsUpdateSpec)
    spec.flags = (_lib.LNS_UPDATE_DECOUPLED_WD if decoupled else 0) | (_lib.LNS_UPDATE_SKIP_NONFINITE if skip_nonfinite else 0)
    spec.lr, spec.beta1, spec.beta2 = float(lr), float(betas[0]), float(betas[1])
    spec.eps, spec.weight_decay, spec.step = float(eps), float(weight_decay), int(step)
    spec.max_norm = 0.0 if max_norm is None else float(max_norm)
    return spec


def _op_check(rc, name):
    """The tail of a call that has no engine handle (lns_op_*, lns_loss_*): the message is the library's create error."""
    if rc != 0:
        raise LnsError("%s failed (%d): %s" % (name, rc, _lib.lib().lns_create_error().decode()))


def _ref(spec):
    """A nullable struct argument."""
    return ctypes.byref(spec) if spec is not None else None


def normalize_obs(obs_steps, weights=None):
    """(steps, weights) of an observation table as plain lists: 0-based, strictly ascending steps, 1 .. LNS_OBS_MAX of them;
    weights finite and >= 0 (None: all 1).  The C calls check the same things; this is the early, readable refusal."""
    import math
    steps = [int(t) for t in obs_steps]
    if not 1 <= len(steps) <= _lib.LNS_OBS_MAX:
        raise LnsError("obs_steps must hold 1 .. %d steps, got %d" % (_lib.LNS_OBS_MAX, len(steps)))
    if steps[0] < 0 or any(b <= a for a, b in zip(steps, steps[1:])):
        raise LnsError("obs_steps must be 0-based and strictly ascending, got %s" % (steps,))
    w = [1.0] * len(steps) if weights is None else [float(v) for v in weights]
    if len(w) != len(steps) or any(not math.isfinite(v) or v < 0 for v in w):
        raise LnsError("weights must be %d finite values >= 0, got %s" % (len(steps), w))
    return steps, w


def fit_spec(obs_steps, weights=None, background=0.0, state=None, param=None):
    """`lns_fit_spec`: the observation table, the weight of the background term, and an update_spec(...) for each of the
    state and `param` that is fitted (None: not fitted).  The host arrays are kept alive by the returned object."""
    steps, w = normalize_obs(obs_steps, weights)
    spec = _lib.LnsFitSpec()
    spec.size = ctypes.sizeof(_lib.LnsFitSpec)
    spec.flags = (_lib.LNS_FIT_STATE if state is not None else 0) | (_lib.LNS_FIT_PARAM if param is not None else 0)
    spec.n_obs = len(steps)
    spec._steps = (ctypes.c_int * len(steps))(*steps)
    spec._weights = (ctypes.c_double * len(w))(*w)
    spec.obs_steps = ctypes.cast(spec._steps, ctypes.POINTER(ctypes.c_int))
    spec.obs_weight = ctypes.cast(spec._weights, ctypes.POINTER(ctypes.c_double))
    spec.background = float(background)
    if state is not None:
        spec.state = state
    if param is not None:
        spec.param = param
    return spec


def gn_spec(obs_steps, weights=None, background=0.0, n_cg=8, damping=0.0, cg_tol=0.0):
    """`lns_gn_spec`: the observation table, the CG steps of one outer Gauss-Newton iteration, the weight of the background
    term, the Levenberg damping mu (absolute, added to the diagonal of H) and the relative residual |r| / |r0| at which a
    sample's CG stops.  The host arrays are kept alive by the returned object."""
    steps, w = normalize_obs(obs_steps, weights)
    spec = _lib.LnsGnSpec()
    spec.size = ctypes.sizeof(_lib.LnsGnSpec)
    spec.flags = 0
    spec.n_obs, spec.n_cg = len(steps), int(n_cg)
    spec._steps = (ctypes.c_int * len(steps))(*steps)
    spec._weights = (ctypes.c_double * len(w))(*w)
    spec.obs_steps = ctypes.cast(spec._steps, ctypes.POINTER(ctypes.c_int))
    spec.obs_weight = ctypes.cast(spec._weights, ctypes.POINTER(ctypes.c_double))
    spec.background, spec.damping, spec.cg_tol = float(background), float(damping), float(cg_tol)
    return spec


def _cg_vectors(who, first, others, scalars, applied=None):
    """The checks cg_start / cg_update share: contiguous fp32 [B,...] HIP tensors of one shape, float64 [B] scalars."""
    import torch
    if not isinstance(first, torch.Tensor) or not first.is_cuda or first.dtype != torch.float32 or first.dim() < 2 \
            or not first.is_contiguous():
        raise LnsError("%s works on contiguous fp32 [B,...] HIP device tensors (there is no CPU fallback), got %s"
                       % (who, ("%s %s on %s" % (first.dtype, tuple(first.shape), first.device)) if isinstance(first, torch.Tensor)
                          else type(first)))
    B = int(first.shape[0])
    for t_ in others:
        if not isinstance(t_, torch.Tensor) or t_.shape != first.shape or t_.dtype != torch.float32 or not t_.is_contiguous() \
                or t_.device != first.device:
            raise LnsError("%s: every vector must be a contiguous fp32 tensor of shape %s on one device" % (who, tuple(first.shape)))
    for t_ in scalars:
        if t_ is not None and (not isinstance(t_, torch.Tensor) or tuple(t_.shape) != (B,) or t_.dtype != torch.float64
                               or not t_.is_contiguous() or t_.device != first.device):
            raise LnsError("%s: rs / rs0 / php must be contiguous float64 [B] tensors on the vectors' device" % who)
    if applied is not None and (tuple(applied.shape) != (B,) or applied.dtype != torch.int32 or not applied.is_contiguous()
                                or applied.device != first.device):
        raise LnsError("%s: applied must be a contiguous int32 [B] tensor on the vectors' device" % who)
    return B, (first[0].numel() if B else 0)


def cg_start(g, x, r, p, rs=None, rs0=None):
    """The start of conjugate gradients per sample (lns_op_cg_start): x = 0, r = p = -g, rs = rs0 = <r, r> in double in a
    fixed order.  g, x, r, p: fp32 [B,...]; rs, rs0: float64 [B] (allocated when None).  Returns (rs, rs0).
    Bit-reproducible; never synchronises.  Module-level because the op needs no engine."""
    import torch
    B, n = _cg_vectors("cg_start", g, (x, r, p), (rs, rs0))
    with torch.cuda.device(g.device):
        rs = torch.empty(B, dtype=torch.float64, device=g.device) if rs is None else rs
        rs0 = torch.empty(B, dtype=torch.float64, device=g.device) if rs0 is None else rs0
        rc = _lib.lib().lns_op_cg_start(g.data_ptr(), x.data_ptr(), r.data_ptr(), p.data_ptr(), B, n, rs.data_ptr(), rs0.data_ptr(),
                                        Engine._stream(g))
    _op_check(rc, "lns_op_cg_start")
    return rs, rs0


def cg_update(x, r, p, hp, rs, rs0, php=None, tol=0.0, applied=None):
    """One step of conjugate gradients per sample (lns_op_cg_update), IN PLACE on x, r, p and rs: hp = H p; php [B] float64:
    <p, H p> (None: <p, hp> is summed inside); a sample whose rs or php is not finite or not positive, or whose
    |r| <= tol |r0|, is not written at all; applied [B] int32: += 1 for every sample that was.  Bit-reproducible; never
    synchronises."""
    import torch
    B, n = _cg_vectors("cg_update", x, (r, p, hp), (rs, rs0, php), applied)
    if rs is None or rs0 is None:
        raise LnsError("cg_update: rs and rs0 are required")
    with torch.cuda.device(x.device):
        rc = _lib.lib().lns_op_cg_update(x.data_ptr(), r.data_ptr(), p.data_ptr(), hp.data_ptr(), Engine._ptr(php), B, n, float(tol),
                                         rs.data_ptr(), rs0.data_ptr(), Engine._ptr(applied), Engine._stream(x))
    _op_check(rc, "lns_op_cg_update")


def obs_loss(z_pred, obs, obs_steps, weights=None, z0=None, z_background=None, background=0.0, need_per=True, need_bg_grad=None,
             grad_out=None):
    """Observation loss of a latent rollout and its gradient, one loss per trajectory (lns_loss_obs_mse): z_pred
    [B,T,c,h,w] (or [B,T,n]), obs [B,n_obs,...] observed at the 0-based steps `obs_steps` with `weights`; z0 and
    z_background [B,...] add background * mean((z0 - z_background)^2).  Returns (loss [B], per [B,n_obs] or None,
    grad_z_pred like z_pred -- exact zeros on the steps that are not observed --, grad_z0_bg like z0 or None).
    grad_out: a buffer for grad_z_pred (every element is written).  Bit-reproducible; never synchronises.  Module-level
    because the op needs no engine."""
    import torch
    z_pred, obs = Engine._dev(z_pred), Engine._dev(obs)
    steps, w = normalize_obs(obs_steps, weights)
    if z_pred.dim() < 3 or obs.dim() != z_pred.dim() or obs.shape[0] != z_pred.shape[0] or obs.shape[1] != len(steps) \
            or obs.shape[2:] != z_pred.shape[2:] or obs.device != z_pred.device:
        raise LnsError("obs must be [B,%d,...] matching z_pred %s on its device, got %s on %s"
                       % (len(steps), tuple(z_pred.shape), tuple(obs.shape), obs.device))
    B, T = int(z_pred.shape[0]), int(z_pred.shape[1])
    n = z_pred[0, 0].numel()
    if (z0 is None) != (z_background is None):
        raise LnsError("z0 and z_background come together (the background term) or not at all")
    if z0 is not None:
        z0, z_background = Engine._dev(z0), Engine._dev(z_background)
        for t_, name in ((z0, "z0"), (z_background, "z_background")):
            if t_.shape[0] != B or t_[0].numel() != n or t_.device != z_pred.device:
                raise LnsError("%s must be [B,...] with %d elements per sample on z_pred's device" % (name, n))
    if need_bg_grad is None:
        need_bg_grad = z0 is not None
    L = _lib.lib()
    nb = ctypes.c_size_t(0)
    rc = L.lns_loss_obs_mse_scratch_bytes(B, len(steps), ctypes.byref(nb))
    if rc == 0:
        with torch.cuda.device(z_pred.device):
            dev = z_pred.device
            loss = torch.empty(B, dtype=torch.float32, device=dev)
            per = torch.empty((B, len(steps)), dtype=torch.float32, device=dev) if need_per else None
            grad = torch.empty_like(z_pred) if grad_out is None else grad_out
            if grad.shape != z_pred.shape or grad.dtype != torch.float32 or not grad.is_contiguous() or grad.device != dev:
                raise LnsError("grad_out must be a contiguous fp32 tensor like z_pred")
            gbg = torch.empty_like(z0) if need_bg_grad else None
            scratch = torch.empty(int(nb.value), dtype=torch.uint8, device=dev)
            rc = L.lns_loss_obs_mse(z_pred.data_ptr(), obs.data_ptr(), B, T, n, len(steps), (ctypes.c_int * len(steps))(*steps),
                                    (ctypes.c_double * len(w))(*w), Engine._ptr(z0), Engine._ptr(z_background), float(background),
                                    Engine._ptr(per), loss.data_ptr(), grad.data_ptr(), Engine._ptr(gbg), scratch.data_ptr(),
                                    scratch.numel(), Engine._stream(z_pred))
    _op_check(rc, "lns_loss_obs_mse")
    return loss, per, grad, gbg


def orthonormalize(v, r_out=None, logr_acc=None, need_r=False):
    """One pass of modified Gram-Schmidt over the K vectors of every sample (lns_op_orthonormalize): v [B,K,...] fp32 is
    orthonormalised IN PLACE, sums in double in a fixed order.  r_out [B,K,K] float64 (or need_r: allocated): the upper
    triangle R of v = Q R; logr_acc [B,K] float64: += log(R_kk).  Returns (v, r_out).  Bit-reproducible; never
    synchronises.  Module-level because the op needs no engine."""
    import torch
    if not isinstance(v, torch.Tensor) or not v.is_cuda or v.dtype != torch.float32 or v.dim() < 3 or not v.is_contiguous():
        raise LnsError("orthonormalize works in place on a contiguous fp32 [B,K,...] HIP device tensor (there is no CPU fallback), "
                       "got %s" % (("%s %s on %s" % (v.dtype, tuple(v.shape), v.device)) if isinstance(v, torch.Tensor) else type(v),))
    B, K = int(v.shape[0]), int(v.shape[1])
    n = v[0, 0].numel() if B and K else 0
    with torch.cuda.device(v.device):
        if need_r and r_out is None:
            r_out = torch.empty((B, K, K), dtype=torch.float64, device=v.device)
        for t_, shape, name in ((r_out, (B, K, K), "r_out"), (logr_acc, (B, K), "logr_acc")):
            if t_ is not None and (tuple(t_.shape) != shape or t_.dtype != torch.float64 or not t_.is_contiguous() or t_.device != v.device):
                raise LnsError("%s must be a contiguous float64 %s tensor on v's device" % (name, shape))
        L = _lib.lib()
        rc = L.lns_op_orthonormalize(v.data_ptr(), B, K, n, Engine._ptr(r_out), Engine._ptr(logr_acc), Engine._stream(v))
    _op_check(rc, "lns_op_orthonormalize")
    return v, r_out


def smooth_l1(pred, target, beta=1.0, need_grad=True, loss_out=None, grad_out=None):
    """F.smooth_l1_loss(pred, target, beta=beta) (train_stage2_ns2d.py:213) and dL/dpred in one pass on the HIP kernel
    (lns_loss_smooth_l1): returns (0-dim device tensor, gradient like pred or None).  Bit-reproducible; never
    synchronises.  Module-level because the op needs no engine; `Engine.smooth_l1` is the same call."""
    import torch
    pred, target = Engine._dev(pred), Engine._dev(target)
    if pred.shape != target.shape or pred.device != target.device:
        raise LnsError("smooth_l1: pred %s on %s and target %s on %s must match"
                       % (tuple(pred.shape), pred.device, tuple(target.shape), target.device))
    L = _lib.lib()
    n = pred.numel()
    with torch.cuda.device(pred.device):
        loss = torch.empty((), dtype=torch.float32, device=pred.device) if loss_out is None else loss_out
        grad = (torch.empty_like(pred) if grad_out is None else grad_out) if need_grad else None
        scratch = torch.empty(max(1, -(-n // _lib.LNS_SL1_CHUNK)), dtype=torch.float32, device=pred.device)
        rc = L.lns_loss_smooth_l1(pred.data_ptr(), target.data_ptr(), n, float(beta), loss.data_ptr(),
                                  grad.data_ptr() if grad is not None else None, scratch.data_ptr(), scratch.numel(),
                                  Engine._stream(pred))
    _op_check(rc, "lns_loss_smooth_l1")
    return loss, grad


def eval_spec(C, mean=0.0, std=1.0, eps=1e-8, zero_wall_channels=(), clamp_channels=(), clamp=(0.0, 1.0 + 1e-8)):
    """`lns_eval_spec` from the arguments of `metrics.relative_l2`, with its rule for the choice between the scalar and
    the per-channel kernel: per-channel as soon as a statistic is a sequence or a channel is zeroed / clamped."""
    spec = _lib.LnsEvalSpec()
    spec.size = ctypes.sizeof(_lib.LnsEvalSpec)
    spec.eps = float(eps)
    spec.clamp_lo, spec.clamp_hi = float(clamp[0]), float(clamp[1])
    per_channel = (not isinstance(mean, (int, float))) or (not isinstance(std, (int, float))) or \
        len(zero_wall_channels) > 0 or len(clamp_channels) > 0
    spec.per_channel = int(per_channel)
    if not per_channel:
        spec.mean, spec.std = float(mean), float(std)
        return spec
    if C > _lib.LNS_METRIC_MAX_CH:
        raise ValueError("per-channel statistics: at most %d channels" % _lib.LNS_METRIC_MAX_CH)

    def per_c(v):
        v = [float(v)] * C if isinstance(v, (int, float)) else [float(e) for e in v]
        if len(v) != C:
            raise ValueError("per-channel statistics need %d entries" % C)
        return v
    m, sd = per_c(mean), per_c(std)
    for c in range(_lib.LNS_METRIC_MAX_CH):
        spec.mean_c[c], spec.std_c[c], spec.flags_c[c] = (m[c], sd[c], 0) if c < C else (0.0, 1.0, 0)
    for c in zero_wall_channels:
        spec.flags_c[c] |= 1
    for c in clamp_channels:
        spec.flags_c[c] |= 2
    return spec


EnsembleScores = collections.namedtuple("EnsembleScores", "rel_l2 rmse spread crps seq rank mean var z_last")
EnsembleScores.__doc__ = """Result of Engine.rollout_latent_ensemble_eval / ensemble_score: rel_l2, rmse, spread, crps
[B, n_keep, C] (views of one [B, n_keep, C, 4] tensor), seq [B, C, 4] (the same four over all kept steps), rank
[B, n_keep, C, M + 1] int32 or None, and mean, var, z_last where asked for (None otherwise)."""


EnsembleQuantiles = collections.namedtuple("EnsembleQuantiles", "quantiles prob mean var z_last")
EnsembleQuantiles.__doc__ = """Result of Engine.rollout_latent_ensemble_quantiles / ensemble_quantiles: quantiles
[B, n_keep, n_q, C, Ly, Lx] (None without a probability), prob [B, n_keep, n_thr, C, Ly, Lx], the share of the members above each
threshold (None without a threshold), and mean, var, z_last where asked for (None otherwise)."""


def quantile_spec(C, members, quantiles=(), thresholds=()):
    """`lns_ensemble_quantile_spec` from the probabilities and the thresholds (each a scalar for every channel, or a
    per-channel sequence); pure host code, so a bad request is refused before any device use."""
    from . import metrics
    quantiles = [float(q) for q in quantiles]
    metrics.quantile_positions(quantiles, max(1, int(members)))           # (refuses a probability outside [0, 1])
    rows = metrics.threshold_table(thresholds, C)
    if len(quantiles) > 8 or len(rows) > 8:
        raise ValueError("at most 8 quantiles and 8 thresholds per call")
    if not quantiles and not rows:
        raise ValueError("neither a quantile nor a threshold was asked for")
    if rows and C > _lib.LNS_METRIC_MAX_CH:
        raise ValueError("thresholds: at most %d channels" % _lib.LNS_METRIC_MAX_CH)
    spec = _lib.LnsEnsembleQuantileSpec()
    spec.size = ctypes.sizeof(_lib.LnsEnsembleQuantileSpec)
    spec.n_q, spec.n_thr = len(quantiles), len(rows)
    for k, q in enumerate(quantiles):
        spec.q[k] = q
    for k, row in enumerate(rows):
        for c, v in enumerate(row):
            spec.thr[k][c] = v
    return spec


EnsembleAnalysis = collections.namedtuple("EnsembleAnalysis", "z param X wbar lam stat status mean var z_last")
EnsembleAnalysis.__doc__ = """Result of Engine.rollout_latent_ensemble_analysis: z [B, M, c, h, w] the analysis latents (the forecast
latents of the last step transformed by X), param [B, M] the transformed per-member param (None unless it was given per
member), X [B, M, M], wbar [B, M], lam [B, M] (the eigenvalues of (M-1)/rho I + S, ascending) and stat [B, n_keep, 3] (the
forecast mean's weighted misfit sum r d^2, sum r, the number of observed values) in float64, status [B] int32 (0 ok, 1 non-finite
Gram, 2 not converged), and (return_mean / return_var / return_last) rollout_latent_ensemble's outputs."""
LocalEnsembleAnalysis = collections.namedtuple(
    "LocalEnsembleAnalysis", "z param X_local wbar_local lam_local status_local X wbar lam stat status mean var z_last")
LocalEnsembleAnalysis.__doc__ = """Result of Engine.rollout_latent_ensemble_analysis_local: z [B, M, c, h, w] the analysis latents (latent
pixel l of the forecast latents of the last step transformed by X_local[:, l]), X_local [B, h*w, M, M], wbar_local and lam_local
[B, h*w, M] (float64), status_local [B, h*w] int32 per domain; param, X, wbar, lam, stat, status: the global transform from the same
patch sums with weight 1 (param: the per-member param it updates, None unless given per member); mean, var, z_last as
EnsembleAnalysis."""
EnsembleExceedance = collections.namedtuple("EnsembleExceedance", "table mean var z_last")
EnsembleExceedance.__doc__ = """Result of Engine.rollout_latent_ensemble_exceed: table [B, n_keep, n_thr, C, 2, M + 1] int32, the
number of a plane's pixels with the truth above the threshold (index 1 of dim 4) or not (index 0) and n of the M members above
it (dim 5); and mean, var, z_last where asked for (None otherwise).  The scores: metrics.brier_scores & co."""


def exceed_spec(C, thresholds):
    """`lns_ensemble_exceed_spec` from the thresholds (each a scalar for every channel, or a per-channel sequence); pure
    host code, so a bad request is refused before any device use."""
    from . import metrics
    rows = metrics.threshold_table(thresholds, C)
    if not 1 <= len(rows) <= 8:
        raise ValueError("between 1 and 8 thresholds per call, got %d" % len(rows))
    if C > _lib.LNS_METRIC_MAX_CH:
        raise ValueError("thresholds: at most %d channels" % _lib.LNS_METRIC_MAX_CH)
    spec = _lib.LnsEnsembleExceedSpec()
    spec.size = ctypes.sizeof(_lib.LnsEnsembleExceedSpec)
    spec.n_thr = len(rows)
    for k, row in enumerate(rows):
        for c, v in enumerate(row):
            spec.thr[k][c] = v
    return spec


EvalSpectra = collections.namedtuple("EvalSpectra", "frame seq frames spectra spectrum_steps")
EvalSpectra.__doc__ = """Result of Engine.rollout_eval_spectrum: frame [B, T, C], seq [B, C] and frames (or None) as rollout_eval
returns them, spectra [B, len(spectrum_steps), C, 3, S] (rows: forecast, truth, error; S = metrics.spectrum_bins(Ly, Lx)) and
spectrum_steps (the list of steps the spectra belong to)."""
EvalSpectraChunk = collections.namedtuple("EvalSpectraChunk", EvalSpectra._fields + ("z_last",))
EvalSpectraChunk.__doc__ = """Result of Engine.rollout_latent_eval_spectrum: EvalSpectra's five fields for the chunk, then z_last, the
latent after the chunk's last step -- appended as rollout_latent_eval appends it to rollout_eval's result."""


EvalStats = collections.namedtuple("EvalStats", "frame seq frames stats hist stats_steps spectra spectrum_steps")
EvalStats.__doc__ = """Result of Engine.rollout_eval_stats: frame [B, T, C], seq [B, C] and frames (or None) as rollout_eval returns
them, stats [B, len(stats_steps), C, 12] (columns: metrics.FIELD_STATS), hist [B, len(stats_steps), C, 2, nbins + 2] int32 (rows
forecast, truth; bins: metrics.histogram_edges) or None, stats_steps, and spectra [B, len(spectrum_steps), C, 3, S] or None with
spectrum_steps (empty: no spectra were asked for)."""
EvalStatsChunk = collections.namedtuple("EvalStatsChunk", EvalStats._fields + ("z_last",))
EvalStatsChunk.__doc__ = """Result of Engine.rollout_latent_eval_stats: EvalStats' fields for the chunk, then z_last, the latent after
the chunk's last step."""


EvalMaps = collections.namedtuple("EvalMaps", EvalStats._fields + ("maps", "map_steps"))
EvalMaps.__doc__ = """Result of Engine.rollout_eval_maps: EvalStats' fields (stats / hist / spectra are None and their step lists empty
where they were not asked for), then maps [B, C, 7, Ly, Lx] (planes: metrics.TIME_MAPS) and map_steps = (from, every), the rule
of the steps the maps were taken over."""
EvalMapsChunk = collections.namedtuple("EvalMapsChunk", EvalMaps._fields + ("z_last",))
EvalMapsChunk.__doc__ = """Result of Engine.rollout_latent_eval_maps: EvalMaps' fields for the chunk, then z_last, the latent after
the chunk's last step.  maps is written by the chunk that completes the horizon."""


# The streaming validation with error attribution (rollout_eval_attrib): frame / seq / frames as rollout_eval; recon_*, prop_*
# and cross_* [B,T,C] / [B,C] with frame^2 = prop^2 + recon^2 + cross; latent_* [B,T] / [B]; recon_frames: the reconstructions
# of keep_steps or None; z_true [B,T,c,h,w] = encode(y) or None.
EvalAttrib = collections.namedtuple("EvalAttrib", "frame seq frames recon_frame recon_seq prop_frame prop_seq cross_frame "
                                    "cross_seq latent_frame latent_seq recon_frames z_true")
EvalAttribChunk = collections.namedtuple("EvalAttribChunk", EvalAttrib._fields + ("z_last",))
# Stage-1 validation (autoencode_eval): frame [B,T,C], seq [B,C], z [B,T,c,h,w] or None
AutoencodeEval = collections.namedtuple("AutoencodeEval", "frame seq z")


def normalize_map_steps(map_steps):
    """The `map_steps` argument of the time maps -> (from, every): None is every step, (0, 1); slice(from, None, every) and a
    (from, every) pair name the steps from, from + every, ... of the horizon (burn-in and thinning).  Anything else -- a stop,
    a negative start, a step below 1, a list of steps -- is a ValueError.  Pure host code."""
    def whole(v, what):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral):
            raise ValueError("map_steps: %s must be an integer, got %r" % (what, v))
        return int(v)
    if map_steps is None:
        return 0, 1
    if isinstance(map_steps, slice):
        if map_steps.stop is not None:
            raise ValueError("map_steps: a slice must be slice(from, None, every): the maps run to the end of the horizon")
        first = 0 if map_steps.start is None else whole(map_steps.start, "from")
        every = 1 if map_steps.step is None else whole(map_steps.step, "every")
    elif isinstance(map_steps, (tuple, list)) and len(map_steps) == 2:
        first, every = whole(map_steps[0], "from"), whole(map_steps[1], "every")
    else:
        raise ValueError("map_steps must be None, slice(from, None, every) or a (from, every) pair, got %r" % (map_steps,))
    if first < 0 or every < 1:
        raise ValueError("map_steps: from must be >= 0 and every >= 1, got (%d, %d)" % (first, every))
    return first, every


def stats_spec(C, hist):
    """`lns_stats_spec` from hist = (nbins, lo, hi) with scalar or per-channel edges (denormalised units); None -> None."""
    if hist is None:
        return None
    nbins, lo, hi = hist
    hs = _lib.LnsStatsSpec()
    hs.size = ctypes.sizeof(_lib.LnsStatsSpec)
    hs.nbins = int(nbins)
    for name, v in (("lo", lo), ("hi", hi)):
        try:                                                            # a number, a numpy scalar or a 0-d array / tensor
            scalar = isinstance(v, numbers.Real) or getattr(v, "ndim", None) == 0
            vals = [float(v)] * min(C, 8) if scalar else [float(e) for e in v]
        except (TypeError, ValueError):
            raise LnsError("hist: %s must be a number or one value per channel (%d), got %r" % (name, C, v))
        if len(vals) != min(C, 8) and len(vals) != C:
            raise LnsError("hist: %s must be a number or one value per channel (%d), got %d" % (name, C, len(vals)))
        for ch, e in enumerate(vals[:8]):
            getattr(hs, name)[ch] = e
    return hs


EvalFlow = collections.namedtuple("EvalFlow", "frame seq frames flow hist vort_frames steps stats stats_hist stats_steps spectra "
                                  "spectrum_steps")
EvalFlow.__doc__ = """Result of Engine.rollout_eval_flow: frame [B, T, C], seq [B, C] and frames (or None) as rollout_eval returns them,
flow [B, len(steps), 12] (columns: metrics.FLOW_STATS), hist [B, len(steps), 2, nbins + 2] int32 (the vorticity of forecast and
truth; bins: metrics.histogram_edges) or None, vort_frames [B, len(keep_steps), Ly, Lx] (the forecast's vorticity of the kept
frames) or None, steps (the steps flow / hist belong to), then rollout_eval_stats' stats / stats_hist / stats_steps and spectra /
spectrum_steps (None and empty where they were not asked for)."""
EvalFlowChunk = collections.namedtuple("EvalFlowChunk", EvalFlow._fields + ("z_last",))
EvalFlowChunk.__doc__ = """Result of Engine.rollout_latent_eval_flow: EvalFlow's fields for the chunk, then z_last, the latent after
the chunk's last step."""


def flow_spec(u=0, v=1, dx=1.0, dy=1.0, boundary="periodic", vort_hist=None, cfg=None):
    """`lns_flow_spec`: the velocity channels u (x-component) and v, the spacings, `boundary` as metrics.flow_boundary takes it
    ("auto" needs cfg) and vort_hist = (nbins, lo, hi) in units of the vorticity or None."""
    from . import metrics
    fs = _lib.LnsFlowSpec()
    fs.size = ctypes.sizeof(_lib.LnsFlowSpec)
    fs.cu, fs.cv = int(u), int(v)
    fs.bc_y, fs.bc_x = metrics.flow_boundary(boundary, cfg)
    fs.dy, fs.dx = float(dy), float(dx)
    if vort_hist is not None:
        try:
            nbins, lo, hi = vort_hist
            fs.nbins, fs.lo, fs.hi = int(nbins), float(lo), float(hi)
        except (TypeError, ValueError):
            raise LnsError("vort_hist must be (nbins, lo, hi) with scalar edges, got %r" % (vort_hist,))
        if not 1 <= fs.nbins <= 256:
            raise LnsError("vort_hist: nbins must be in 1 .. 256, got %d" % fs.nbins)
    return fs


def normalize_keep_steps(keep_steps, steps):
    """The `keep_steps` argument of the selected-step rollout -> list of ints, strictly ascending, in [0, steps).
    A slice is resolved against `steps` as indexing a [.., steps, ..] tensor would (slice(None, None, 5) is `::5`); a
    range or any sequence of integers is taken as it is.  Pure host code; LnsError names what is wrong."""
    import operator
    steps = int(steps)
    if steps <= 0:
        raise LnsError("steps must be positive, got %d" % steps)
    if isinstance(keep_steps, slice):
        keep = list(range(*keep_steps.indices(steps)))
    else:
        try:
            keep = [operator.index(s) for s in keep_steps]
        except TypeError:
            raise LnsError("keep_steps must be a sequence of ints, a range or a slice, got %r" % (keep_steps,))
    if not keep:
        raise LnsError("keep_steps selects no step of the %d (for latents only: to_x=False)" % steps)
    for i, s in enumerate(keep):
        if s < 0 or s >= steps or (i > 0 and s <= keep[i - 1]):
            raise LnsError("keep_steps must be ascending steps in [0, %d): entry %d is %d" % (steps, i, s))
    return keep


class Engine:
    """One lns_engine handle (one per GPU; not thread-safe)."""

    def __init__(self, cfg: LnsConfig):
        L = _lib.lib()
        self._L = L
        self.cfg = cfg
        h = ctypes.c_void_p()
        rc = L.lns_create(ctypes.byref(cfg), ctypes.byref(h))
        if rc != 0:
            raise LnsError("lns_create failed: %s" % L.lns_create_error().decode())
        self._h = h
        self._ws = {}
        self.options = {}                     # what set_option was given (options never set are at the library's defaults)
        self.device_index = None
        self.params = self._param_table()

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                self._L.lns_destroy(h)
            except Exception:
                pass

    def _check(self, rc, what):
        if rc != 0:
            raise LnsError("%s failed (%d): %s" % (what, rc, self._L.lns_last_error(self._h).decode()))

    def _param_table(self):
        out = []
        n = self._L.lns_num_params(self._h)
        key = ctypes.create_string_buffer(_lib_key_cap())
        shape = (ctypes.c_int64 * 8)()
        nd, isb = ctypes.c_int(), ctypes.c_int()
        for i in range(n):
            self._check(self._L.lns_param_info(self._h, i, key, len(key), shape, ctypes.byref(nd),
                                               ctypes.byref(isb)), "lns_param_info")
            out.append((key.value.decode(), tuple(int(shape[j]) for j in range(nd.value)), bool(isb.value)))
        return out

    def param_shapes(self):
        return {k: s for k, s, _ in self.params}

    # -- weights ---------------------------------------------------------------
    def load_weights(self, weights: dict, device_index: int):
        """weights: {key: float32 ndarray}; all keys of the table must be present."""
        for key, shape, _ in self.params:
            if key not in weights:
                raise KeyError("missing key in state_dict: %s" % key)
            a = np.ascontiguousarray(weights[key], dtype=np.float32)
            if tuple(a.shape) != tuple(shape):
                raise ValueError("size mismatch for %s: %s vs %s" % (key, a.shape, shape))
            shp = (ctypes.c_int64 * 8)(*shape)
            self._check(self._L.lns_set_weight(self._h, key.encode(), a.ctypes.data_as(ctypes.c_void_p),
                                               shp, len(shape)), "lns_set_weight")
        self._check(self._L.lns_finalize_weights(self._h, int(device_index)), "lns_finalize_weights")
        self.device_index = int(device_index)
        self._ws.clear()

    def set_option(self, name, value):
        """Scheduling options of the rollout (include/lns.h lns_set_option): decode_group, decode_streams, overlap,
        prop_priority, track_nonfinite, fa_chunk_mb, fa_fused_gpb, eval_max_steps (longest horizon of rollout_eval; it sizes
        the evaluation workspace), train_wgrad (0: one block per output tile, 1: batch-parallel weight gradient of the
        training step; it sizes the training workspaces, and the gradients differ by the summation order only).
        Results never depend on the others.  "fa_fused" (default 2; 1 = single-buffered kernel, same bits; 0 = off) selects
        the arithmetic form of FABlock2D at 64 x 64 planes (in_proj inside the sandwich kernel): ~2e-7 relative on the fields.
        "fold_linear" (default 1; 0 = off) runs a convolution directly followed by a 1x1 convolution as one convolution on
        weights composed at load_weights: the same order of difference.
        "up2_dual" (default 1; 0 = the per-phase form everywhere) picks the kernel form of the upsampling 3x3 convolutions:
        the same bits either way.
        "spectrum_basis" (default 0; basis_y | basis_x << 1, 0 = dft, 1 = dct) selects which energy spectrum the streaming
        calls compute; their basis= / spectrum_basis= keywords set it for one call and put it back."""
        self._check(self._L.lns_set_option(self._h, name.encode(), int(value)), "lns_set_option")
        self.options[name] = int(value)
        self._ws.clear()                      # the workspace size depends on the options

    def latent_shape(self):
        c, h, w = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        self._check(self._L.lns_latent_shape(self._h, ctypes.byref(c), ctypes.byref(h), ctypes.byref(w)),
                    "lns_latent_shape")
        return c.value, h.value, w.value

    # -- execution ---------------------------------------------------------------
    def _workspace(self, B, device, min_bytes=0):
        import torch
        n = ctypes.c_size_t(0)
        if self.cfg.ae_kind != LNS_AE_NONE:
            self._check(self._L.lns_prepare(self._h, int(B), ctypes.byref(n)), "lns_prepare")
        need = max(int(n.value), int(min_bytes), 1 << 20)
        ws = self._ws.get((B, device))
        if ws is None or ws.numel() < need:
            ws = torch.empty(need, dtype=torch.uint8, device=device)
            self._ws[(B, device)] = ws
        return ws

    @staticmethod
    def _stream(t):
        """The current HIP stream of the device `t` lives on (not of whatever device is current)."""
        import torch
        return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)

    def _param(self, param, like):
        """Conditional propagator: one normalised parameter per trajectory -> fp32 [B] on like's device."""
        import torch
        if param is None:
            return None
        B = like.shape[0]
        p = torch.as_tensor(param)
        if p.numel() != B:
            raise LnsError("param must hold one value per trajectory: got %d values for batch %d" % (p.numel(), B))
        if p.device != like.device:
            raise LnsError("param is on %s but the fields are on %s" % (p.device, like.device))
        return p.reshape(B).to(torch.float32).contiguous()

    @staticmethod
    def _dev(t):
        import torch
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise LnsError("the LNS engine runs on HIP device tensors only (got %s); there is no CPU "
                           "fallback" % (t.device if hasattr(t, "device") else type(t)))
        if t.dtype != torch.float32:
            raise LnsError("fp32 tensors expected, got %s" % t.dtype)
        return t.contiguous()

    def encode(self, x, param=None, scale_shift=None):
        """scale_shift [B, in_channels, 2] (device): encode(x * scale + shift) with the affine map applied in the first
        convolution's prologue (lns_encode_affine; the dataset normalisation of encode_dataset)."""
        import torch
        x = self._dev(x)
        B = x.shape[0]
        C, H, W = self.latent_shape()
        z = torch.empty((B, C, H, W), dtype=torch.float32, device=x.device)
        ws = self._workspace(B, x.device)
        if scale_shift is not None:
            ss = self._dev(scale_shift)
            if tuple(ss.shape) != (B, self.cfg.in_channels, 2) or ss.device != x.device:
                raise LnsError("scale_shift must be [B, in_channels, 2] on the input's device")
            if bool(self.cfg.cond_encoder) != (param is not None):
                raise LnsError("param must be given exactly for a conditional encoder")
            p = self._param(param, x) if param is not None else None
            self._check(self._L.lns_encode_affine(self._h, x.data_ptr(), ss.data_ptr(), self._ptr(p),
                                                  B, z.data_ptr(), ws.data_ptr(), ws.numel(), self._stream(x)),
                        "lns_encode_affine")
            return z
        if self.cfg.cond_encoder:
            if param is None:
                raise LnsError("this autoencoder's encoder is conditional: encode(x, param)")
            p = self._param(param, x)
            self._check(self._L.lns_encode_cond(self._h, x.data_ptr(), p.data_ptr(), B, z.data_ptr(), ws.data_ptr(),
                                                ws.numel(), self._stream(x)), "lns_encode_cond")
            return z
        self._check(self._L.lns_encode(self._h, x.data_ptr(), B, z.data_ptr(), ws.data_ptr(), ws.numel(),
                                       self._stream(x)), "lns_encode")
        return z

    def decode(self, z):
        import torch
        z = self._dev(z)
        B = z.shape[0]
        c = self.cfg
        y = torch.empty((B, c.in_channels, c.Ly, c.Lx), dtype=torch.float32, device=z.device)
        ws = self._workspace(B, z.device)
        self._check(self._L.lns_decode(self._h, z.data_ptr(), B, y.data_ptr(), ws.data_ptr(), ws.numel(),
                                       self._stream(z)), "lns_decode")
        return y

    def propagate(self, z, param=None):
        import torch
        z = self._dev(z)
        B, C, H, W = z.shape
        out = torch.empty_like(z)
        p = self._param(param, z)
        # propagator-only engines have no lns_prepare(): size generously from the activations
        ws = self._workspace(B, z.device, min_bytes=64 * B * max(C, self.cfg.prop_n_embd) * H * W * 4 + (1 << 22))
        self._check(self._L.lns_propagate(self._h, z.data_ptr(), self._ptr(p),
                                          B, H, W, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                          self._stream(z)), "lns_propagate")
        return out

    def _sized_workspace(self, query, B, device):
        """The engine's workspace for batch B, at least as large as the size query `query` (lns_*_workspace_bytes) asks."""
        n = ctypes.c_size_t(0)
        self._check(getattr(self._L, query)(self._h, int(B), ctypes.byref(n)), query)
        return self._workspace(B, device, min_bytes=int(n.value))

    @staticmethod
    def _ptr(t):
        return t.data_ptr() if t is not None else None

    @staticmethod
    def _out(out, shape, device):
        """A new fp32 tensor of `shape`, or the caller's preallocated one once it is seen to fit."""
        import torch
        if out is None:
            return torch.empty(shape, dtype=torch.float32, device=device)
        if tuple(out.shape) != shape or not out.is_contiguous():
            raise LnsError("preallocated output must be contiguous with shape %s" % (shape,))
        return out

    @staticmethod
    def _keep_array(steps, to_x, keep_steps):
        """keep_steps of rollout / rollout_latent -> ctypes int array (pure host code: decided before any device use)."""
        if not to_x:
            raise LnsError("keep_steps selects the steps to DECODE; for latents slice the latent rollout "
                           "(rollout(..., to_x=False)[:, keep_steps]): every latent is computed anyway")
        keep = normalize_keep_steps(keep_steps, steps)
        return (ctypes.c_int * len(keep))(*keep)

    def _rollout_call(self, first, from_x, steps, param, to_x, out, keep_steps, want_side):
        """The one call behind rollout (from_x: `first` is x) and rollout_latent (`first` is z), with every step or with
        keep_steps -> (out, side output): all latents [B, steps, C, H, W] from x, the latent after the last step from z."""
        import contextlib
        import torch
        B = first.shape[0]
        c = self.cfg
        C, H, W = self.latent_shape()
        keep = self._keep_array(steps, to_x, keep_steps) if keep_steps is not None else None
        if not to_x:
            shape = (B, steps, C, H, W)
        else:
            shape = (B, steps if keep is None else len(keep), c.in_channels, c.Ly, c.Lx)
        out = self._out(out, shape, first.device)
        side = torch.empty((B, steps, C, H, W) if from_x else tuple(first.shape), dtype=torch.float32,
                           device=first.device) if want_side else None
        p = self._param(param, first)
        name = "lns_rollout" + ("" if from_x else "_latent") + ("" if keep is None else "_select")
        sink = (int(bool(to_x)), out.data_ptr()) if keep is None else (keep, len(keep), out.data_ptr())
        # the selected-step calls run with the input's device current, the others with whatever device the caller has
        with torch.cuda.device(first.device) if keep is not None else contextlib.nullcontext():
            if keep is None:
                ws = self._workspace(B, first.device)
            else:
                ws = self._sized_workspace("lns_rollout_select_workspace_bytes", B, first.device)
            self._check(getattr(self._L, name)(self._h, first.data_ptr(), self._ptr(p), B, int(steps), *sink, self._ptr(side),
                                               ws.data_ptr(), ws.numel(), self._stream(first)), name)
        return out, side

    def rollout(self, x, steps, param=None, to_x=True, return_latents=False, out=None, keep_steps=None):
        """keep_steps (a sequence of ints, a range, or a slice resolved against `steps`: slice(None, None, 5) is the
        reference's y_hat[:, ::5]): decode these steps only -> [B, n_keep, C, Ly, Lx], the bits of rollout(x, steps)[:, keep_steps]
        without the decodes, or the memory, of the other steps.  return_latents still gives all `steps` latents."""
        out, lat = self._rollout_call(self._dev(x), True, steps, param, to_x, out, keep_steps, return_latents)
        return (out, lat) if return_latents else out

    def rollout_latent(self, z, steps, param=None, to_x=True, out=None, keep_steps=None):
        """Continue from latent z: returns (out [B,steps,...], z after the last step).  keep_steps (steps of this chunk,
        as for `rollout`): out is [B, n_keep, C, Ly, Lx]."""
        return self._rollout_call(self._dev(z), False, steps, param, to_x, out, keep_steps, True)

    # -- ensemble rollout (include/lns.h "ensemble rollout") -------------------------------------------------------
    @staticmethod
    def _member_param(param, z, B, M):
        """param of an ensemble call: one value per trajectory [B] (broadcast over the members) or per member -> fp32 [B, M]."""
        import torch
        if param is None:
            return None
        p = torch.as_tensor(param)
        if p.device != z.device:
            raise LnsError("param is on %s but the latents are on %s" % (p.device, z.device))
        if p.numel() == B:
            p = p.reshape(B, 1).expand(B, M)
        elif p.numel() != B * M:
            raise LnsError("param must hold one value per trajectory or per member: got %d values for B = %d, M = %d"
                           % (p.numel(), B, M))
        return p.reshape(B, M).to(torch.float32).contiguous()

    def _ensemble_setup(self, z, steps, keep_steps, return_mean, return_var, few=None, y=None, y_obs=None):
        """The checks the six rollout_latent_ensemble* methods share, in the order they are made, and what follows from them:
        a record of z, B, M, steps, keep, arr (keep as a ctypes array), nk, tail = (C, Ly, Lx) and y, the truth of the kept
        steps; mean, var, z_last and p are `_ensemble_outputs`'.  The truth comes as y [B, T, ...] (steps None: T; the kept steps
        are sliced out) or as y_obs [B, n_keep, ...] (taken as it is).  few: the text of the refusal of a variance of fewer than
        two members, for the forms that refuse it here."""
        import torch
        z = self._dev(z)
        truth = y if y is not None else y_obs
        if truth is not None:
            truth = self._dev(truth)
        C, H, W = self.latent_shape()
        c = self.cfg
        tail = (c.in_channels, c.Ly, c.Lx)
        if z.dim() != 5 or tuple(z.shape[2:]) != (C, H, W):
            raise LnsError("ensemble latents must be [B, M, %d, %d, %d], got %s" % (C, H, W, tuple(z.shape)))
        B, M = int(z.shape[0]), int(z.shape[1])

        def flags():
            if return_var and not return_mean:
                raise LnsError("return_var needs return_mean (the variance comes from the kernel that writes the mean)")
            if few and return_var and M < 2:
                raise LnsError(few % M)
        if y is not None:
            if truth.dim() != 5 or truth.shape[0] != B or tuple(truth.shape[2:]) != tail or truth.dtype != torch.float32:
                raise LnsError("ground truth must be fp32 [B, T, %d, %d, %d] with the latents' batch, got %s" % (tail + (tuple(truth.shape),)))
            if truth.device != z.device:
                raise LnsError("ground truth is on %s but the latents are on %s" % (truth.device, z.device))
        if y_obs is None:
            flags()
        steps = int(truth.shape[1]) if steps is None and y is not None else int(steps)
        if y is not None and steps > truth.shape[1]:
            raise LnsError("%d steps do not fit the %d steps of the ground truth" % (steps, truth.shape[1]))
        keep = normalize_keep_steps(range(steps) if keep_steps is None else keep_steps, steps)
        nk = len(keep)
        if y_obs is not None:
            if tuple(truth.shape) != (B, nk) + tail or truth.device != z.device:
                raise LnsError("y_obs must be %s on the latents' device, got %s" % ((B, nk) + tail, tuple(truth.shape)))
            flags()
        if y is not None:
            truth = truth[:, keep].contiguous()
        return types.SimpleNamespace(z=z, B=B, M=M, steps=steps, keep=keep, arr=(ctypes.c_int * nk)(*keep), nk=nk, tail=tail, y=truth,
                                     mean=None, var=None, z_last=None, p=None)

    def _ensemble_outputs(self, s, param, return_mean, return_var, return_last, out=None):
        """mean (out: the caller's), var and z_last where asked for and the per-member param into the record -- behind whatever the
        form makes of its own arguments, so that a bad request is refused before a bad param."""
        import torch
        shape = (s.B, s.nk) + s.tail
        s.mean = self._out(out, shape, s.z.device) if return_mean else None
        s.var = torch.empty(shape, dtype=torch.float32, device=s.z.device) if return_var else None
        s.z_last = torch.empty_like(s.z) if return_last else None
        s.p = self._member_param(param, s.z, s.B, s.M)

    def _ensemble_workspace(self, B, M, device, query="lns_rollout_ensemble_workspace_bytes", *args):
        """The workspace of batch B * M, at least as large as the ensemble size query `query` asks."""
        n = ctypes.c_size_t(0)
        self._check(getattr(self._L, query)(self._h, B, M, *args, ctypes.byref(n)), query)
        return self._workspace(B * M, device, min_bytes=int(n.value))

    def rollout_latent_ensemble(self, z, steps, param=None, keep_steps=None, return_var=True, return_last=False, out=None):
        """z [B, M, c, h, w]: M perturbed members of each of B trajectories (the noise is the caller's, as in training).
        Rolls every member out and returns, per kept step, the mean and the unbiased variance over the members
        [B, n_keep, C, Ly, Lx] without storing the members' fields: `mean`, or `(mean, var)`, with `z_last` [B, M, c, h, w]
        appended under return_last.  keep_steps as for `rollout` (None: every step).  param: one value per trajectory
        [B] (broadcast over the members) or per member [B, M].  M = 1 has no variance: return_var=False.  out: a
        preallocated mean.  The workspace is the one of batch B * M: `check_finite(B * M)` covers the call."""
        import torch
        s = self._ensemble_setup(z, steps, keep_steps, True, return_var,
                                 few="the variance needs at least 2 members, got M = %d (return_var=False for the mean alone)")
        self._ensemble_outputs(s, param, True, return_var, return_last, out)
        with torch.cuda.device(s.z.device):
            ws = self._ensemble_workspace(s.B, s.M, s.z.device)
            self._check(self._L.lns_rollout_latent_ensemble(self._h, s.z.data_ptr(), self._ptr(s.p), s.B, s.M, s.steps, s.arr, s.nk,
                                                            s.mean.data_ptr(), self._ptr(s.var), self._ptr(s.z_last), ws.data_ptr(),
                                                            ws.numel(), self._stream(s.z)), "lns_rollout_latent_ensemble")
        res = (s.mean,) + ((s.var,) if return_var else ()) + ((s.z_last,) if return_last else ())
        return res[0] if len(res) == 1 else res

    def ensemble_stats(self, frames, return_var=True):
        """The reduction kernel of the ensemble rollout on its own: frames [B, M, ...] -> mean [B, ...] or (mean, var)
        (unbiased, over dim 1) in the fixed order documented in include/lns.h (lns_op_ensemble_stats)."""
        import torch
        if not isinstance(frames, torch.Tensor) or not frames.is_cuda or frames.dtype != torch.float32 or frames.dim() < 2:
            raise LnsError("ensemble_stats takes an fp32 HIP tensor [B, M, ...]")
        if not frames.is_contiguous():
            frames = frames.contiguous()
        B, M = int(frames.shape[0]), int(frames.shape[1])
        per = frames[0, 0].numel() if frames.dim() > 2 else 1
        shape = (B,) + tuple(frames.shape[2:])
        mean = torch.empty(shape, dtype=torch.float32, device=frames.device)
        var = torch.empty(shape, dtype=torch.float32, device=frames.device) if return_var else None
        with torch.cuda.device(frames.device):
            rc = self._L.lns_op_ensemble_stats(frames.data_ptr(), B, M, per, mean.data_ptr(), self._ptr(var), self._stream(frames))
        _op_check(rc, "lns_op_ensemble_stats")
        return (mean, var) if return_var else mean

    # -- ensemble validation (include/lns.h "ensemble validation") ---------------------------------------------------
    @staticmethod
    def _scores_result(scores, seq, rank, mean=None, var=None, z_last=None):
        return EnsembleScores(scores[..., 0], scores[..., 1], scores[..., 2], scores[..., 3], seq, rank, mean, var, z_last)

    @staticmethod
    def _frames_and_truth(op, frames, y, yname):
        """frames [n, B, M, C, H, W] and the truth [B, n, C, H, W] of an op wrapper, checked -> (frames, truth, frames' shape)."""
        import torch
        for t in (frames, y):
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
                raise LnsError("%s takes fp32 HIP tensors" % op)
        if frames.dim() != 6 or y.dim() != 5 or y.device != frames.device:
            raise LnsError("%s takes frames [n, B, M, C, H, W] and %s [B, n, C, H, W] on one device" % (op, yname))
        n, B, M, C, H, W = shape = tuple(int(v) for v in frames.shape)
        if tuple(y.shape) != (B, n, C, H, W):
            raise LnsError("%s must be %s for frames %s, got %s" % (yname, (B, n, C, H, W), shape, tuple(y.shape)))
        return frames.contiguous(), y.contiguous(), shape

    def ensemble_score(self, frames, y, return_rank=True, **norm):
        """The scoring kernels of the ensemble validation on stored member fields (lns_op_ensemble_score): frames
        [n, B, M, C, H, W] (a frame buffer's layout), y [B, n, C, H, W], both normalised; `norm` as in `rollout_eval`.
        Returns EnsembleScores (mean, var, z_last None)."""
        import torch
        frames, y, (n, B, M, C, H, W) = self._frames_and_truth("ensemble_score", frames, y, "y")
        spec = eval_spec(C, **norm)
        scores = torch.empty((B, n, C, 4), dtype=torch.float32, device=y.device)
        seq = torch.empty((B, C, 4), dtype=torch.float32, device=y.device)
        rank = torch.empty((B, n, C, M + 1), dtype=torch.int32, device=y.device) if return_rank else None
        with torch.cuda.device(y.device):
            rc = self._L.lns_op_ensemble_score(frames.data_ptr(), y.data_ptr(), n, B, M, C, H, W, ctypes.byref(spec),
                                               scores.data_ptr(), seq.data_ptr(), self._ptr(rank), None, self._stream(y))
        _op_check(rc, "lns_op_ensemble_score")
        return self._scores_result(scores, seq, rank)

    def rollout_latent_ensemble_eval(self, z, y, steps=None, param=None, keep_steps=None, return_rank=True, return_mean=False,
                                     return_var=False, return_last=False, **norm):
        """rollout_latent_ensemble with the members scored against the truth as they are decoded: z [B, M, c, h, w] as there
        (2 <= M <= 128), y [B, T, C, Ly, Lx] the normalised truth of all `steps` = T steps (the kept ones, y[:, keep_steps],
        are what is scored; keep_steps None: every step), `norm` as in `rollout_eval`.  Returns EnsembleScores: per kept
        step and channel the relative L2 error and the RMSE of the ensemble mean, the spread (root of the mean unbiased
        member variance) and the fair CRPS, their sequence-wise forms, the rank histogram of the truth among the members,
        and (return_mean / return_var / return_last) rollout_latent_ensemble's outputs.  The member fields are never stored;
        the workspace is rollout_latent_ensemble's."""
        import torch
        s = self._ensemble_setup(z, steps, keep_steps, return_mean, return_var, y=y)
        C, dev = self.cfg.in_channels, s.z.device
        spec = eval_spec(C, **norm)
        scores = torch.empty((s.B, s.nk, C, 4), dtype=torch.float32, device=dev)
        seq = torch.empty((s.B, C, 4), dtype=torch.float32, device=dev)
        rank = torch.empty((s.B, s.nk, C, s.M + 1), dtype=torch.int32, device=dev) if return_rank else None
        self._ensemble_outputs(s, param, return_mean, return_var, return_last)
        with torch.cuda.device(dev):
            ws = self._ensemble_workspace(s.B, s.M, dev)
            self._check(self._L.lns_rollout_latent_ensemble_eval(
                self._h, s.z.data_ptr(), self._ptr(s.p), s.y.data_ptr(), s.B, s.M, s.steps, s.arr, s.nk, ctypes.byref(spec),
                scores.data_ptr(), seq.data_ptr(), self._ptr(rank), self._ptr(s.mean), self._ptr(s.var), self._ptr(s.z_last),
                ws.data_ptr(), ws.numel(), self._stream(s.z)), "lns_rollout_latent_ensemble_eval")
        return self._scores_result(scores, seq, rank, s.mean, s.var, s.z_last)

    # -- ensemble quantiles (include/lns.h "ensemble quantiles") -------------------------------------------------------
    def ensemble_quantiles(self, frames, quantiles=(), thresholds=(), **norm):
        """The quantile kernel on stored member fields (lns_op_ensemble_quantiles): frames [n, B, M, C, H, W] (a frame
        buffer's layout), normalised; quantiles: probabilities in [0, 1]; thresholds: each a scalar (every channel) or a
        per-channel sequence, in the units of the denormalised values; `norm` as in `rollout_eval` (none: the values as they
        are).  Returns EnsembleQuantiles (mean, var, z_last None)."""
        import torch
        if not isinstance(frames, torch.Tensor) or not frames.is_cuda or frames.dtype != torch.float32 or frames.dim() != 6:
            raise LnsError("ensemble_quantiles takes an fp32 HIP tensor [n, B, M, C, H, W]")
        n, B, M, C, H, W = (int(v) for v in frames.shape)
        frames = frames.contiguous()
        qs = quantile_spec(C, M, quantiles, thresholds)
        spec = eval_spec(C, **norm) if norm else None
        quant = torch.empty((B, n, qs.n_q, C, H, W), dtype=torch.float32, device=frames.device) if qs.n_q else None
        prob = torch.empty((B, n, qs.n_thr, C, H, W), dtype=torch.float32, device=frames.device) if qs.n_thr else None
        with torch.cuda.device(frames.device):
            rc = self._L.lns_op_ensemble_quantiles(frames.data_ptr(), n, B, M, C, H, W, ctypes.byref(qs), _ref(spec),
                                                   self._ptr(quant), self._ptr(prob), self._stream(frames))
        _op_check(rc, "lns_op_ensemble_quantiles")
        return EnsembleQuantiles(quant, prob, None, None, None)

    def rollout_latent_ensemble_quantiles(self, z, steps, quantiles=(0.05, 0.5, 0.95), thresholds=(), param=None, keep_steps=None,
                                          return_mean=False, return_var=False, return_last=False, **norm):
        """rollout_latent_ensemble with, per kept step and pixel, quantiles of the member values and the share of the members
        above each threshold, taken as the members are decoded: z [B, M, c, h, w] as there (1 <= M <= 128); quantiles:
        probabilities in [0, 1] (numpy's "linear" definition; 0 / 1: the member minimum / maximum); thresholds: each a scalar
        (every channel) or a per-channel sequence, in the units of the values; `norm` as in `rollout_eval` -- without it the
        values are normalised, as the mean is.  Returns EnsembleQuantiles; return_mean / return_var / return_last add
        rollout_latent_ensemble's outputs.  The member fields are never stored; the workspace is rollout_latent_ensemble's."""
        import torch
        s = self._ensemble_setup(z, steps, keep_steps, return_mean, return_var, few="the variance needs at least 2 members, got M = %d")
        C, dev = self.cfg.in_channels, s.z.device
        qs = quantile_spec(C, s.M, quantiles, thresholds)
        spec = eval_spec(C, **norm) if norm else None
        quant = torch.empty((s.B, s.nk, qs.n_q) + s.tail, dtype=torch.float32, device=dev) if qs.n_q else None
        prob = torch.empty((s.B, s.nk, qs.n_thr) + s.tail, dtype=torch.float32, device=dev) if qs.n_thr else None
        self._ensemble_outputs(s, param, return_mean, return_var, return_last)
        with torch.cuda.device(dev):
            ws = self._ensemble_workspace(s.B, s.M, dev)
            self._check(self._L.lns_rollout_latent_ensemble_quantiles(
                self._h, s.z.data_ptr(), self._ptr(s.p), s.B, s.M, s.steps, s.arr, s.nk, ctypes.byref(qs), _ref(spec), self._ptr(quant),
                self._ptr(prob), self._ptr(s.mean), self._ptr(s.var), self._ptr(s.z_last), ws.data_ptr(), ws.numel(), self._stream(s.z)),
                "lns_rollout_latent_ensemble_quantiles")
        return EnsembleQuantiles(quant, prob, s.mean, s.var, s.z_last)

    # -- ensemble exceedance tables (include/lns.h "ensemble exceedance") ---------------------------------------------
    def ensemble_exceed(self, frames, y, thresholds, **norm):
        """The counting kernel of the exceedance tables on stored member fields (lns_op_ensemble_exceed): frames
        [n, B, M, C, H, W] (a frame buffer's layout), y [B, n, C, H, W], both normalised; thresholds: each a scalar (every
        channel) or a per-channel sequence, in the units of the denormalised values; `norm` as in `rollout_eval` (none: the
        values as they are).  Returns the int32 table [B, n, n_thr, C, 2, M + 1]."""
        import torch
        frames, y, (n, B, M, C, H, W) = self._frames_and_truth("ensemble_exceed", frames, y, "y")
        xs = exceed_spec(C, thresholds)
        spec = eval_spec(C, **norm) if norm else None
        table = torch.empty((B, n, xs.n_thr, C, 2, M + 1), dtype=torch.int32, device=y.device)
        with torch.cuda.device(y.device):
            rc = self._L.lns_op_ensemble_exceed(frames.data_ptr(), y.data_ptr(), n, B, M, C, H, W, ctypes.byref(xs), _ref(spec),
                                                table.data_ptr(), self._stream(y))
        _op_check(rc, "lns_op_ensemble_exceed")
        return table

    def rollout_latent_ensemble_exceed(self, z, y, steps, thresholds, param=None, keep_steps=None, return_mean=False,
                                       return_var=False, return_last=False, **norm):
        """rollout_latent_ensemble with, per kept step, threshold and channel, the contingency table of the event "value above
        the threshold": how many of the plane's pixels had n of the M members above it while the truth was (1) or was not (0)
        above it, counted as the members are decoded.  z [B, M, c, h, w] as there (1 <= M <= 128), y [B, T, C, Ly, Lx] the
        normalised truth of all `steps` = T steps (None: y.shape[1]; the kept ones, y[:, keep_steps], are what is compared);
        thresholds: each a scalar (every channel) or a per-channel sequence, in the units of the values; `norm` as in
        `rollout_eval` -- without it members and truth are compared in normalised units.  Returns EnsembleExceedance;
        return_mean / return_var / return_last add rollout_latent_ensemble's outputs.  The member fields are never stored;
        the workspace is rollout_latent_ensemble's.  The scores are functions of the table: metrics.brier_scores,
        reliability_curve, roc_curve, contingency_scores."""
        import torch
        s = self._ensemble_setup(z, steps, keep_steps, return_mean, return_var, few="the variance needs at least 2 members, got M = %d", y=y)
        C, dev = self.cfg.in_channels, s.z.device
        xs = exceed_spec(C, thresholds)
        spec = eval_spec(C, **norm) if norm else None
        table = torch.empty((s.B, s.nk, xs.n_thr, C, 2, s.M + 1), dtype=torch.int32, device=dev)
        self._ensemble_outputs(s, param, return_mean, return_var, return_last)
        with torch.cuda.device(dev):
            ws = self._ensemble_workspace(s.B, s.M, dev)
            self._check(self._L.lns_rollout_latent_ensemble_exceed(
                self._h, s.z.data_ptr(), self._ptr(s.p), s.y.data_ptr(), s.B, s.M, s.steps, s.arr, s.nk, ctypes.byref(xs), _ref(spec),
                table.data_ptr(), self._ptr(s.mean), self._ptr(s.var), self._ptr(s.z_last), ws.data_ptr(), ws.numel(), self._stream(s.z)),
                "lns_rollout_latent_ensemble_exceed")
        return EnsembleExceedance(table, s.mean, s.var, s.z_last)

    # -- ensemble transform Kalman filter (include/lns.h "ensemble transform Kalman filter") --------------------------
    @staticmethod
    def _rinv(rinv, B, n, tail, device):
        """rinv [C, H, W] (shared), [n, C, H, W] (per step) or [B, n, C, H, W] -> (fp32 contiguous tensor, batch stride, step
        stride) as lns_op_ensemble_obs_gram addresses it."""
        import torch
        if not isinstance(rinv, torch.Tensor) or not rinv.is_cuda or rinv.dtype != torch.float32 or rinv.device != device:
            raise LnsError("rinv must be an fp32 HIP tensor on the device of the fields")
        per = int(tail[0] * tail[1] * tail[2])
        shape = tuple(rinv.shape)
        if shape == tuple(tail):
            return rinv.contiguous(), 0, 0
        if shape == (n,) + tuple(tail):
            return rinv.contiguous(), 0, per
        if shape == (B, n) + tuple(tail):
            return rinv.contiguous(), n * per, per
        raise LnsError("rinv must be %s, %s or %s, got %s" % (tuple(tail), (n,) + tuple(tail), (B, n) + tuple(tail), shape))

    def ensemble_obs_gram(self, frames, y_obs, rinv, **norm):
        """The Gram kernel of the ensemble Kalman filter on stored member fields (lns_op_ensemble_obs_gram): frames
        [n, B, M, C, H, W] (a frame buffer's layout), y_obs [B, n, C, H, W], both normalised; rinv: the inverse
        observation-error variance per value, [C, H, W], [n, C, H, W] or [B, n, C, H, W] (0: not observed); `norm` as in
        `rollout_eval` (none: the values as they are).  Returns (S [B, n, M, M], g [B, n, M], stat [B, n, 3]) in float64."""
        import torch
        frames, y_obs, (n, B, M, C, H, W) = self._frames_and_truth("ensemble_obs_gram", frames, y_obs, "y_obs")
        r, r_bs, r_ss = self._rinv(rinv, B, n, (C, H, W), frames.device)
        spec = eval_spec(C, **norm) if norm else None
        S = torch.empty((B, n, M, M), dtype=torch.float64, device=frames.device)
        g = torch.empty((B, n, M), dtype=torch.float64, device=frames.device)
        stat = torch.empty((B, n, 3), dtype=torch.float64, device=frames.device)
        with torch.cuda.device(frames.device):
            rc = self._L.lns_op_ensemble_obs_gram(frames.data_ptr(), y_obs.data_ptr(), r.data_ptr(), r_bs, r_ss, n, B, M, C, H, W,
                                                  _ref(spec), S.data_ptr(), g.data_ptr(), stat.data_ptr(), self._stream(frames))
        _op_check(rc, "lns_op_ensemble_obs_gram")
        return S, g, stat

    def etkf_transform(self, S, g, rho=1.0):
        """The transform kernel of the filter (lns_op_etkf_transform): S [B, n, M, M], g [B, n, M] float64 (summed over the n
        steps) and the multiplicative inflation rho >= 1 -> (X [B, M, M], wbar [B, M], lam [B, M] ascending, status [B] int32:
        0 ok, 1 non-finite Gram (that sample's X is NaN), 2 not converged).  Nothing is read back."""
        import torch
        for t in (S, g):
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float64:
                raise LnsError("etkf_transform takes float64 HIP tensors")
        if S.dim() != 4 or S.shape[2] != S.shape[3] or tuple(g.shape) != tuple(S.shape[:3]) or g.device != S.device:
            raise LnsError("etkf_transform takes S [B, n, M, M] and g [B, n, M] on one device, got %s and %s" % (tuple(S.shape), tuple(g.shape)))
        B, n, M = (int(v) for v in S.shape[:3])
        S, g = S.contiguous(), g.contiguous()
        X = torch.empty((B, M, M), dtype=torch.float64, device=S.device)
        wbar = torch.empty((B, M), dtype=torch.float64, device=S.device)
        lam = torch.empty((B, M), dtype=torch.float64, device=S.device)
        status = torch.empty((B,), dtype=torch.int32, device=S.device)
        with torch.cuda.device(S.device):
            rc = self._L.lns_op_etkf_transform(S.data_ptr(), g.data_ptr(), B, n, M, float(rho), X.data_ptr(), wbar.data_ptr(),
                                               lam.data_ptr(), status.data_ptr(), self._stream(S))
        _op_check(rc, "lns_op_etkf_transform")
        return X, wbar, lam, status

    def ensemble_transform(self, z, X, out=None):
        """The update kernel of the filter (lns_op_ensemble_transform): z [B, M, ...] fp32, X [B, M, M] float64 -> the members
        transformed about their mean, out_m = zbar + sum_k (z_k - zbar) X_km; out may be z itself.  [B, M] is the update of
        a per-member param."""
        import torch
        if not isinstance(z, torch.Tensor) or not z.is_cuda or z.dtype != torch.float32 or z.dim() < 2 or not z.is_contiguous():
            raise LnsError("ensemble_transform takes a contiguous fp32 HIP tensor [B, M, ...]")
        B, M = int(z.shape[0]), int(z.shape[1])
        if not isinstance(X, torch.Tensor) or X.dtype != torch.float64 or X.device != z.device or tuple(X.shape) != (B, M, M):
            raise LnsError("X must be float64 %s on the device of z, got %s" % ((B, M, M), tuple(getattr(X, "shape", ()))))
        if out is None:
            out = torch.empty_like(z)
        elif out.shape != z.shape or out.dtype != z.dtype or out.device != z.device or not out.is_contiguous():
            raise LnsError("out must be a contiguous tensor of z's shape, dtype and device")
        n = z[0, 0].numel() if z.dim() > 2 else 1
        with torch.cuda.device(z.device):
            rc = self._L.lns_op_ensemble_transform(z.data_ptr(), X.contiguous().data_ptr(), B, M, n, out.data_ptr(), self._stream(z))
        _op_check(rc, "lns_op_ensemble_transform")
        return out

    def _analysis_outputs(self, s, param):
        """What both analysis methods return of the global filter: za, pa (the transformed param: given per member only), X, wbar,
        lam, stat, status."""
        import torch
        f64 = dict(dtype=torch.float64, device=s.z.device)
        per_member = s.p is not None and torch.as_tensor(param).numel() == s.B * s.M and s.M > 1
        return (torch.empty_like(s.z), torch.empty_like(s.p) if per_member else None, torch.empty((s.B, s.M, s.M), **f64),
                torch.empty((s.B, s.M), **f64), torch.empty((s.B, s.M), **f64), torch.empty((s.B, s.nk, 3), **f64),
                torch.empty((s.B,), dtype=torch.int32, device=s.z.device))

    def rollout_latent_ensemble_analysis(self, z, y_obs, rinv, steps, param=None, keep_steps=None, rho=1.0, return_mean=False,
                                         return_var=False, return_last=False, **norm):
        """One window of the ensemble transform Kalman filter: rollout_latent_ensemble over `steps` steps with the decoded
        members compared with sparse observations as they are decoded, and the forecast latents of the last step corrected
        by them.  z [B, M, c, h, w] (2 <= M <= 64); keep_steps: the observed steps (None: every step); y_obs
        [B, n_keep, C, Ly, Lx]: the normalised observations of those steps (any value where rinv is 0); rinv [C, Ly, Lx],
        [n_keep, C, Ly, Lx] or [B, n_keep, C, Ly, Lx]: the inverse observation-error variance in the units of the values
        (`norm` as in `rollout_eval`; none: normalised units); rho >= 1: the multiplicative inflation; param: per trajectory
        or per member -- given per member ([B, M]) it is updated by the same transform.  Returns EnsembleAnalysis.  The
        member fields are never stored and nothing is read back."""
        import torch
        s = self._ensemble_setup(z, steps, keep_steps, return_mean, return_var, y_obs=y_obs)
        dev = s.z.device
        r, r_bs, r_ss = self._rinv(rinv, s.B, s.nk, s.tail, dev)
        spec = eval_spec(self.cfg.in_channels, **norm) if norm else None
        self._ensemble_outputs(s, param, return_mean, return_var, return_last)
        za, pa, X, wbar, lam, stat, status = self._analysis_outputs(s, param)
        with torch.cuda.device(dev):
            ws = self._ensemble_workspace(s.B, s.M, dev, "lns_rollout_ensemble_analysis_workspace_bytes", s.nk)
            self._check(self._L.lns_rollout_latent_ensemble_analysis(
                self._h, s.z.data_ptr(), self._ptr(s.p), s.y.data_ptr(), r.data_ptr(), r_bs, r_ss, s.B, s.M, s.steps, s.arr, s.nk,
                _ref(spec), float(rho), za.data_ptr(), self._ptr(pa), X.data_ptr(), wbar.data_ptr(), lam.data_ptr(), stat.data_ptr(),
                status.data_ptr(), self._ptr(s.mean), self._ptr(s.var), self._ptr(s.z_last), ws.data_ptr(), ws.numel(),
                self._stream(s.z)), "lns_rollout_latent_ensemble_analysis")
        return EnsembleAnalysis(za, pa, X, wbar, lam, stat, status, s.mean, s.var, s.z_last)

    # -- localised ensemble transform Kalman filter (include/lns.h "localised ensemble transform Kalman filter") ------
    def ensemble_patch_gram(self, frames, y_obs, rinv, grid, **norm):
        """The patch Gram kernel of the localised filter on stored member fields (lns_op_ensemble_patch_gram): frames, y_obs, rinv
        and `norm` as `ensemble_obs_gram`; grid = (h, w): the latent grid whose patches cut the frame.  Returns part
        [B, n, h*w, M*M + M + 3] float64: per patch the Gram [M, M] (symmetric), g [M] and stat [3]."""
        import torch
        frames, y_obs, (n, B, M, C, H, W) = self._frames_and_truth("ensemble_patch_gram", frames, y_obs, "y_obs")
        h, w = (int(v) for v in grid)
        r, r_bs, r_ss = self._rinv(rinv, B, n, (C, H, W), frames.device)
        spec = eval_spec(C, **norm) if norm else None
        part = torch.empty((B, n, max(h * w, 0), M * M + M + 3), dtype=torch.float64, device=frames.device)
        with torch.cuda.device(frames.device):
            rc = self._L.lns_op_ensemble_patch_gram(frames.data_ptr(), y_obs.data_ptr(), r.data_ptr(), r_bs, r_ss, n, B, M, C, H, W, h, w,
                                                    _ref(spec), part.data_ptr(), self._stream(frames))
        _op_check(rc, "lns_op_ensemble_patch_gram")
        return part

    def letkf_combine(self, part, grid, radius, boundary=("periodic", "periodic")):
        """The combine kernel of the localised filter (lns_op_letkf_combine): part [B, n, h*w, M*M + M + 3] float64, grid = (h, w),
        radius: the Gaspari-Cohn half-width in latent pixels, boundary: as metrics.flow_boundary (not "auto") -> (S_local
        [B, h*w, M, M], g_local [B, h*w, M], S_glob [B, M, M], g_glob [B, M], stat [B, n, 3]) in float64."""
        import torch
        from . import metrics
        h, w = (int(v) for v in grid)
        if not isinstance(part, torch.Tensor) or not part.is_cuda or part.dtype != torch.float64 or part.dim() != 4 or part.shape[2] != h * w:
            raise LnsError("letkf_combine takes a float64 HIP tensor [B, n, h*w, M*M + M + 3]")
        B, n, hw, E = (int(v) for v in part.shape)
        M = int(round((-1 + (1 + 4 * (E - 3)) ** 0.5) / 2))
        if M * M + M + 3 != E:
            raise LnsError("the last axis of part must be M*M + M + 3, got %d" % E)
        bc_y, bc_x = metrics.flow_boundary(boundary)
        part = part.contiguous()
        f64 = dict(dtype=torch.float64, device=part.device)
        S_l, g_l = torch.empty((B, hw, M, M), **f64), torch.empty((B, hw, M), **f64)
        S_g, g_g, stat = torch.empty((B, M, M), **f64), torch.empty((B, M), **f64), torch.empty((B, n, 3), **f64)
        with torch.cuda.device(part.device):
            rc = self._L.lns_op_letkf_combine(part.data_ptr(), B, n, M, h, w, float(radius), bc_y, bc_x, S_l.data_ptr(), g_l.data_ptr(),
                                              S_g.data_ptr(), g_g.data_ptr(), stat.data_ptr(), self._stream(part))
        _op_check(rc, "lns_op_letkf_combine")
        return S_l, g_l, S_g, g_g, stat

    def ensemble_transform_local(self, z, X_local, out=None):
        """The update kernel of the localised filter (lns_op_ensemble_transform_local): z [B, M, c, h, w] fp32, X_local
        [B, h*w, M, M] float64 -> latent pixel l of every channel transformed by X_local[:, l]; out may be z itself."""
        import torch
        if not isinstance(z, torch.Tensor) or not z.is_cuda or z.dtype != torch.float32 or z.dim() != 5 or not z.is_contiguous():
            raise LnsError("ensemble_transform_local takes a contiguous fp32 HIP tensor [B, M, c, h, w]")
        B, M, c, h, w = (int(v) for v in z.shape)
        if not isinstance(X_local, torch.Tensor) or X_local.dtype != torch.float64 or X_local.device != z.device or \
                tuple(X_local.shape) != (B, h * w, M, M):
            raise LnsError("X_local must be float64 %s on the device of z, got %s" % ((B, h * w, M, M), tuple(getattr(X_local, "shape", ()))))
        if out is None:
            out = torch.empty_like(z)
        elif out.shape != z.shape or out.dtype != z.dtype or out.device != z.device or not out.is_contiguous():
            raise LnsError("out must be a contiguous tensor of z's shape, dtype and device")
        with torch.cuda.device(z.device):
            rc = self._L.lns_op_ensemble_transform_local(z.data_ptr(), X_local.contiguous().data_ptr(), B, M, c, h, w, out.data_ptr(),
                                                         self._stream(z))
        _op_check(rc, "lns_op_ensemble_transform_local")
        return out

    def rollout_latent_ensemble_analysis_local(self, z, y_obs, rinv, steps, loc_radius, boundary="auto", param=None, keep_steps=None,
                                               rho=1.0, return_mean=False, return_var=False, return_last=False, return_X=True, **norm):
        """One window of the localised filter: rollout_latent_ensemble_analysis with one transform per latent pixel.  loc_radius:
        the Gaspari-Cohn half-width in latent pixels (the weights vanish at 2 loc_radius); boundary: "auto" (the model's padding
        per axis), "periodic", "wall" or a pair (y, x), as metrics.flow_boundary; return_X = False leaves X_local, wbar_local in
        the workspace.  Everything else as rollout_latent_ensemble_analysis.  Returns LocalEnsembleAnalysis."""
        import torch
        from . import metrics
        s = self._ensemble_setup(z, steps, keep_steps, return_mean, return_var, y_obs=y_obs)
        dev = s.z.device
        bc_y, bc_x = metrics.flow_boundary(boundary, self.cfg)
        r, r_bs, r_ss = self._rinv(rinv, s.B, s.nk, s.tail, dev)
        spec = eval_spec(self.cfg.in_channels, **norm) if norm else None
        self._ensemble_outputs(s, param, return_mean, return_var, return_last)
        za, pa, X, wbar, lam, stat, status = self._analysis_outputs(s, param)
        f64 = dict(dtype=torch.float64, device=dev)
        hw = s.z.shape[3] * s.z.shape[4]
        Xl = torch.empty((s.B, hw, s.M, s.M), **f64) if return_X else None
        wl = torch.empty((s.B, hw, s.M), **f64) if return_X else None
        ll = torch.empty((s.B, hw, s.M), **f64)
        sl = torch.empty((s.B, hw), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            ws = self._ensemble_workspace(s.B, s.M, dev, "lns_rollout_ensemble_analysis_local_workspace_bytes", s.nk)
            self._check(self._L.lns_rollout_latent_ensemble_analysis_local(
                self._h, s.z.data_ptr(), self._ptr(s.p), s.y.data_ptr(), r.data_ptr(), r_bs, r_ss, s.B, s.M, s.steps, s.arr, s.nk,
                _ref(spec), float(rho), float(loc_radius), bc_y, bc_x, za.data_ptr(), self._ptr(Xl), self._ptr(wl), ll.data_ptr(),
                sl.data_ptr(), self._ptr(pa), X.data_ptr(), wbar.data_ptr(), lam.data_ptr(), stat.data_ptr(), status.data_ptr(),
                self._ptr(s.mean), self._ptr(s.var), self._ptr(s.z_last), ws.data_ptr(), ws.numel(), self._stream(s.z)),
                "lns_rollout_latent_ensemble_analysis_local")
        return LocalEnsembleAnalysis(za, pa, Xl, wl, ll, sl, X, wbar, lam, stat, status, s.mean, s.var, s.z_last)

    # -- streaming validation rollout (include/lns.h "streaming validation rollout") --------------------------------
    def _eval_common(self, first, y, steps, t0, keep_steps, norm):
        """Shared argument handling of rollout_eval / rollout_latent_eval -> (y, B, T, T_total, spec, keep array, frames)."""
        import torch
        y = self._dev(y)
        c = self.cfg
        if y.dim() != 5 or y.shape[0] != first.shape[0] or tuple(y.shape[2:]) != (c.in_channels, c.Ly, c.Lx):
            raise LnsError("ground truth must be [B, T, %d, %d, %d] with the input's batch, got %s"
                           % (c.in_channels, c.Ly, c.Lx, tuple(y.shape)))
        if y.device != first.device:
            raise LnsError("ground truth is on %s but the input is on %s" % (y.device, first.device))
        B, T_total = int(y.shape[0]), int(y.shape[1])
        T = T_total - t0 if steps is None else int(steps)
        if t0 < 0 or T <= 0 or t0 + T > T_total:
            raise LnsError("steps %d from step %d do not fit the %d steps of the ground truth" % (T, t0, T_total))
        spec = eval_spec(c.in_channels, **norm)
        keep = [int(s) for s in keep_steps]
        arr = (ctypes.c_int * len(keep))(*keep) if keep else None
        frames = torch.empty((B, len(keep), c.in_channels, c.Ly, c.Lx), dtype=torch.float32, device=y.device) if keep else None
        return y, B, T, T_total, spec, arr, len(keep), frames

    @staticmethod
    def _result(t, shape, device):
        """A new fp32 result tensor of `shape`, or the caller's preallocated one once it is seen to fit."""
        import torch
        if t is None:
            return torch.empty(shape, dtype=torch.float32, device=device)
        if tuple(t.shape) != shape or not t.is_contiguous() or t.dtype != torch.float32 or t.device != device:
            raise LnsError("preallocated result must be a contiguous fp32 tensor of shape %s on the input's device" % (shape,))
        return t

    def _scored_call(self, name, result, first, y, steps, t0, param, keep_steps, norm, select=None, frame=None, seq=None,
                     maps=None, attrib=None):
        """The one body behind the eight scored rollouts: C entry point `name`, from x (t0 None: `first` is x, steps < T
        scores the first `steps` of y) or continued from a latent at step t0 (`first` is z; frame / seq / maps may be the
        caller's).  select(T, B, device) -> (the entry point's arguments after the stream, the result's fields after
        `frames`, the lns_eval_select whose maps this call owns or None); `result` builds what is returned from
        frame, seq, frames, those fields, [maps, map_steps] and, from a latent, z_last.  attrib(B, T_total, device, frames) ->
        (lns_eval_attrib, the result's fields after `frames`): the attribution forms, whose struct stands in front of the workspace."""
        import torch
        latent = t0 is not None
        first = self._dev(first)
        if latent:
            t0 = int(t0)
        elif steps is not None and int(steps) < y.shape[1]:
            y = y[:, :int(steps)]
        y, B, T, T_total, spec, keep, n_keep, frames = self._eval_common(first, y, steps, t0 if latent else 0, keep_steps, norm)
        extra, tail, q = select(T, B, first.device) if select is not None else ((), (), None)
        c = self.cfg
        frame = self._result(frame, (B, T_total, c.in_channels), first.device)
        seq = self._result(seq, (B, c.in_channels), first.device)
        query = "lns_rollout_eval_workspace_bytes"
        if q is not None:
            maps = self._result(maps, (B, c.in_channels, _lib.LNS_TIME_MAPS, c.Ly, c.Lx), first.device)
            q.maps_out = maps.data_ptr()
            tail += (maps, (q.map_from, q.map_every))
            query = "lns_rollout_eval_maps_workspace_bytes"
        front = ()
        if attrib is not None:
            at, atail = attrib(B, T_total, first.device, frames)
            front, tail, query = (ctypes.byref(at),), tail + atail, "lns_rollout_eval_attrib_workspace_bytes"
        z_last = torch.empty_like(first) if latent else None
        p = self._param(param, first)
        with torch.cuda.device(first.device):
            ws = self._sized_workspace(query, B, first.device)
            self._check(getattr(self._L, name)(
                self._h, first.data_ptr(), self._ptr(p), y.data_ptr(), B, T, *((t0, T_total) if latent else ()),
                ctypes.byref(spec), frame.data_ptr(), seq.data_ptr(), keep, n_keep, self._ptr(frames),
                *((z_last.data_ptr(),) if latent else ()), *front, ws.data_ptr(), ws.numel(), self._stream(first), *extra), name)
        return result(frame, seq, frames, *tail, *((z_last,) if latent else ()))

    def rollout_eval(self, x, y, steps=None, param=None, keep_steps=(), **norm):
        """The validation loop's predict -> denormalize -> relative_lp_loss pair (train_stage2_ns2d.py:249-263) without the
        [B,T,C,Ly,Lx] rollout: every decoded group of steps is scored against the normalised ground truth y [B,T,C,Ly,Lx]
        right after its decode.  `norm`: mean / std / eps / zero_wall_channels / clamp_channels / clamp as in
        `metrics.relative_l2` (so `**metrics.twophase_spec(...)` works).  steps < T scores the first `steps` of y.
        Returns (frame_wise [B,T,C], seq_wise [B,C], frames [B,len(keep_steps),C,Ly,Lx] or None): the same bits as
        `metrics.relative_l2(rollout(x, T), y, ...)` and `rollout(x, T)[:, keep_steps]`."""
        return self._scored_call("lns_rollout_eval", lambda *r: r, x, y, steps, None, param, keep_steps, norm)

    def rollout_latent_eval(self, z, y, steps=None, t0=0, param=None, keep_steps=(), frame=None, seq=None, **norm):
        """rollout_eval continued from a latent: scores steps t0 .. t0+steps-1 of y [B,T_total,C,Ly,Lx] (steps=None: to
        the end).  Chunks of one evaluation must follow each other on the same engine and batch: their per-plane sums
        stay in the engine's workspace, and the call that completes the horizon (t0 + steps == T_total) writes `frame`
        [B,T_total,C] and `seq` [B,C] (pass the tensors along, or take them from the last chunk's return value).
        keep_steps are relative to the chunk.  Returns (frame, seq, frames or None, z after the last step)."""
        return self._scored_call("lns_rollout_latent_eval", lambda *r: r, z, y, steps, t0, param, keep_steps, norm,
                                 frame=frame, seq=seq)

    # -- streaming validation with energy spectra (include/lns.h "energy spectra") ----------------------------------
    def spectrum_bins(self, H=None, W=None, basis="dft"):
        """Number of shells S of an H x W plane (default: the model's Ly x Lx) under `basis` ("dft", "dct", a pair (y, x) or
        "auto": see metrics.spectrum_basis); host only."""
        H, W = (self.cfg.Ly if H is None else int(H)), (self.cfg.Lx if W is None else int(W))
        from . import metrics
        return metrics.spectrum_bins(H, W, self._basis_names(basis))

    def _basis_names(self, basis):
        """`basis` with "auto" resolved against this model, as a pair of names; host only, a bad name raises LnsError."""
        from . import metrics
        by, bx = metrics.spectrum_basis(basis, self.cfg)
        return metrics.SPECTRUM_BASES[by], metrics.SPECTRUM_BASES[bx]

    @contextlib.contextmanager
    def _spectrum_basis(self, basis):
        """The option "spectrum_basis" (include/lns.h: which spectrum the streaming calls compute) set for one call and put
        back afterwards.  It sizes no workspace, so the cached workspaces stay."""
        from . import metrics
        by, bx = metrics.spectrum_basis(basis, self.cfg)
        code, old = by | bx << 1, self.options.get("spectrum_basis", 0)
        if code != old:
            self._check(self._L.lns_set_option(self._h, b"spectrum_basis", code), "lns_set_option")
            self.options["spectrum_basis"] = code
        try:
            yield (metrics.SPECTRUM_BASES[by], metrics.SPECTRUM_BASES[bx])
        finally:
            if code != old:
                self._check(self._L.lns_set_option(self._h, b"spectrum_basis", old), "lns_set_option")
                self.options["spectrum_basis"] = old

    def _spectrum_select(self, spectrum_steps, T, B, device, optional=False, basis="dft"):
        """A `select` of _scored_call: the spectra of `spectrum_steps`; optional: an empty sequence asks for none."""
        import torch
        if optional and spectrum_steps is not None and not isinstance(spectrum_steps, slice) and len(spectrum_steps) == 0:
            return (None, 0, None), (None, []), None
        sel = normalize_keep_steps(range(T) if spectrum_steps is None else spectrum_steps, T)
        arr = (ctypes.c_int * len(sel))(*sel)
        spectra = torch.empty((B, len(sel), self.cfg.in_channels, 3, self.spectrum_bins(basis=basis)), dtype=torch.float32, device=device)
        return (arr, len(sel), spectra.data_ptr()), (spectra, sel), None

    def energy_spectrum(self, y_hat, y=None, basis="dft", **norm):
        """Shell-summed energy spectra of stored fields (lns_op_energy_spectrum): y_hat and y (optional) [B, T, C, H, W],
        normalised; `norm` as in `rollout_eval` (eps is not used).  Returns [B, T, C, 3, S] (forecast, truth, error = forecast -
        truth differenced before the transform) or, without y, [B, T, C, 1, S]: the kernel body of rollout_eval_spectrum.
        `basis`: "dft", "dct", a pair (y, x), or "auto" ("dct" on the axes this model's autoencoder does not pad circularly)."""
        from . import metrics
        return metrics.energy_spectrum(y_hat, y, basis=self._basis_names(basis), **norm)

    def rollout_eval_spectrum(self, x, y, steps=None, param=None, keep_steps=(), spectrum_steps=None, basis="dft", **norm):
        """rollout_eval with the energy spectra of forecast, truth and error of the steps `spectrum_steps` (what
        `normalize_keep_steps` takes; None: every step), taken where the step is decoded.  Returns EvalSpectra: frame, seq
        and frames hold rollout_eval's bits, spectra [B, n, C, 3, S] those of
        `energy_spectrum(rollout(x, T)[:, spectrum_steps], y[:, spectrum_steps], ...)`.  Bins are index wavenumbers; under
        basis="dft" a spectrum of a non-periodic family carries the leakage of the walls: pass basis="auto" (or "dct" / a pair
        (y, x)) for a DCT-II on the axes with walls, S = spectrum_bins(basis=basis) bins at metrics.spectrum_wavenumbers.
        The workspace is rollout_eval's."""
        with self._spectrum_basis(basis) as names:
            return self._scored_call("lns_rollout_eval_spectrum", EvalSpectra, x, y, steps, None, param, keep_steps, norm,
                                     functools.partial(self._spectrum_select, spectrum_steps, basis=names))

    def rollout_latent_eval_spectrum(self, z, y, steps=None, t0=0, param=None, keep_steps=(), spectrum_steps=None, frame=None,
                                     seq=None, basis="dft", **norm):
        """rollout_latent_eval with energy spectra: keep_steps and spectrum_steps are relative to the chunk, spectra
        [B, n, C, 3, S] belong to this chunk's steps.  Returns EvalSpectraChunk (see rollout_latent_eval for frame / seq)."""
        with self._spectrum_basis(basis) as names:
            return self._scored_call("lns_rollout_latent_eval_spectrum", EvalSpectraChunk, z, y, steps, t0, param, keep_steps, norm,
                                     functools.partial(self._spectrum_select, spectrum_steps, basis=names), frame, seq)

    # -- streaming validation with field statistics (include/lns.h "field statistics") ----------------------------
    def field_stats(self, y_hat, y, hist=None, **norm):
        """Per-plane statistics of stored fields (lns_op_field_stats): see metrics.field_stats.  The kernel body of
        rollout_eval_stats."""
        from . import metrics
        return metrics.field_stats(y_hat, y, hist=hist, **norm)

    def _stats_alloc(self, stats_steps, hist, T, B, device):
        """-> (stats steps, their array, stats, lns_stats_spec or None, hist or None)"""
        import torch
        C = self.cfg.in_channels
        sel = normalize_keep_steps(range(T) if stats_steps is None else stats_steps, T)
        arr = (ctypes.c_int * len(sel))(*sel)
        stats = torch.empty((B, len(sel), C, _lib.LNS_FIELD_STATS), dtype=torch.float32, device=device)
        hs = stats_spec(C, hist)
        counts = None
        if hs is not None:
            if not 1 <= hs.nbins <= 256:
                raise LnsError("hist: nbins must be in 1 .. 256, got %d" % hs.nbins)
            counts = torch.empty((B, len(sel), C, 2, hs.nbins + 2), dtype=torch.int32, device=device)
        return sel, arr, stats, hs, counts

    def _stats_select(self, stats_steps, hist, spectrum_steps, T, B, device, basis="dft"):
        """A `select` of _scored_call: the statistics of `stats_steps`, their histograms and (optional) spectra."""
        sel, arr, stats, hs, counts = self._stats_alloc(stats_steps, hist, T, B, device)
        sargs, stail, _ = self._spectrum_select(spectrum_steps, T, B, device, optional=True, basis=basis)
        hp = _ref(hs)
        return sargs + (arr, len(sel), hp, stats.data_ptr(), self._ptr(counts)), (stats, counts, sel) + stail, None

    def rollout_eval_stats(self, x, y, steps=None, param=None, keep_steps=(), stats_steps=None, hist=None, spectrum_steps=(),
                           spectrum_basis="dft", **norm):
        """rollout_eval with, for the steps `stats_steps` (what `normalize_keep_steps` takes; None: every step), the twelve
        per-plane statistics metrics.FIELD_STATS of the decoded frame against the truth -- means, variances, centred
        correlation, the reference's pointwise_correlation, the gradient-domain relative L2 in y and x, and the extrema -- and,
        with hist = (nbins, lo, hi) (scalar or per-channel edges, denormalised units), the value histograms of both.
        `spectrum_steps` (default: none; None: every step) adds rollout_eval_spectrum's spectra in the same pass.  Returns
        EvalStats: frame, seq, frames and spectra hold the bits of the existing calls, stats / hist those of
        `field_stats(rollout(x, T)[:, stats_steps], y[:, stats_steps], hist, ...)`.  The workspace is rollout_eval's."""
        with self._spectrum_basis(spectrum_basis) as names:
            return self._scored_call("lns_rollout_eval_stats", EvalStats, x, y, steps, None, param, keep_steps, norm,
                                     functools.partial(self._stats_select, stats_steps, hist, spectrum_steps, basis=names))

    def rollout_latent_eval_stats(self, z, y, steps=None, t0=0, param=None, keep_steps=(), stats_steps=None, hist=None,
                                  spectrum_steps=(), frame=None, seq=None, spectrum_basis="dft", **norm):
        """rollout_latent_eval with field statistics: keep_steps, stats_steps and spectrum_steps are relative to the chunk,
        stats / hist / spectra belong to this chunk's steps.  Returns EvalStatsChunk (see rollout_latent_eval for frame / seq)."""
        with self._spectrum_basis(spectrum_basis) as names:
            return self._scored_call("lns_rollout_latent_eval_stats", EvalStatsChunk, z, y, steps, t0, param, keep_steps, norm,
                                     functools.partial(self._stats_select, stats_steps, hist, spectrum_steps, basis=names), frame, seq)

    # -- streaming validation with time maps (include/lns.h "time maps") -------------------------------------------
    def time_maps(self, y_hat, y, map_steps=None, **norm):
        """Per-pixel time maps of stored fields (lns_op_time_maps): see metrics.time_maps.  The kernel body of
        rollout_eval_maps."""
        from . import metrics
        return metrics.time_maps(y_hat, y, map_steps=map_steps, **norm)

    def _select_struct(self, stats_steps, hist, spectrum_steps, T, B, device, basis="dft"):
        """-> (an lns_eval_select with the (optional) statistics and spectra, EvalStats' fields after `frames`)"""
        q = _lib.LnsEvalSelect()
        q.size = ctypes.sizeof(_lib.LnsEvalSelect)
        tail = (None, None, [])
        if stats_steps is not None and not isinstance(stats_steps, slice) and len(stats_steps) == 0:
            if hist is not None:
                raise LnsError("hist needs stats_steps")
        else:
            sel, arr, stats, hs, counts = self._stats_alloc(stats_steps, hist, T, B, device)
            q.n_stats, q.stats_steps_host, q.stats_out = len(sel), arr, stats.data_ptr()
            if hs is not None:
                q.hspec, q.hist_out = ctypes.pointer(hs), counts.data_ptr()
            tail = (stats, counts, sel)
        (sarr, n_spec, spectra), stail, _ = self._spectrum_select(spectrum_steps, T, B, device, optional=True, basis=basis)
        if n_spec:
            q.n_spec, q.spectrum_steps_host, q.spectra_out = n_spec, sarr, spectra
        return q, tail + stail

    def _maps_select(self, map_steps, stats_steps, hist, spectrum_steps, T, B, device, basis="dft"):
        """A `select` of _scored_call: the lns_eval_select of the time maps over `map_steps` = (from, every) with the
        (optional) statistics and spectra; the maps tensor itself is _scored_call's."""
        q, tail = self._select_struct(stats_steps, hist, spectrum_steps, T, B, device, basis)
        q.map_from, q.map_every = map_steps
        return (ctypes.byref(q),), tail, q

    def rollout_eval_maps(self, x, y, steps=None, param=None, keep_steps=(), map_steps=None, stats_steps=(), hist=None,
                          spectrum_steps=(), spectrum_basis="dft", **norm):
        """rollout_eval with the seven per-pixel time maps metrics.TIME_MAPS -- time-mean of forecast and truth, their unbiased
        temporal variances and covariance, the mean squared error and the largest absolute error -- over the steps `map_steps`
        (None: every step; slice(from, None, every) or (from, every): burn-in and thinning), accumulated as the steps are decoded:
        the [B,T,C,Ly,Lx] rollout is never stored.  `stats_steps` / `hist` and `spectrum_steps` (default: none) add
        rollout_eval_stats' statistics and rollout_eval_spectrum's spectra in the same pass.  Returns EvalMaps: every field but
        maps holds the bits of the existing calls, maps those of `time_maps(rollout(x, T), y, map_steps, ...)`.  The workspace is
        rollout_eval's plus 52 bytes per (trajectory, channel, pixel)."""
        ms = normalize_map_steps(map_steps)
        with self._spectrum_basis(spectrum_basis) as names:
            return self._scored_call("lns_rollout_eval_maps", EvalMaps, x, y, steps, None, param, keep_steps, norm,
                                     functools.partial(self._maps_select, ms, stats_steps, hist, spectrum_steps, basis=names))

    def rollout_latent_eval_maps(self, z, y, steps=None, t0=0, param=None, keep_steps=(), map_steps=None, stats_steps=(),
                                 hist=None, spectrum_steps=(), frame=None, seq=None, maps=None, spectrum_basis="dft", **norm):
        """rollout_latent_eval with time maps: `map_steps` names steps of the horizon (the same in every chunk); keep_steps,
        stats_steps and spectrum_steps are relative to the chunk.  The chunks of one horizon must follow each other on the same
        engine and batch, with nothing else run on it in between: the maps' state stays in the engine's workspace, and the chunk
        that completes the horizon writes `maps` (pass the tensor along like frame / seq, or take it from the last chunk's
        result; it is untouched until then).  Returns EvalMapsChunk."""
        ms = normalize_map_steps(map_steps)
        with self._spectrum_basis(spectrum_basis) as names:
            return self._scored_call("lns_rollout_latent_eval_maps", EvalMapsChunk, z, y, steps, t0, param, keep_steps, norm,
                                     functools.partial(self._maps_select, ms, stats_steps, hist, spectrum_steps, basis=names), frame, seq, maps)

    # -- streaming validation with flow diagnostics (include/lns.h "flow diagnostics") -----------------------------
    def _boundary_names(self, boundary):
        """`boundary` with "auto" resolved against this model, as a pair of names; host only, a bad name raises LnsError."""
        from . import metrics
        by, bx = metrics.flow_boundary(boundary, self.cfg)
        return metrics.FLOW_BOUNDARIES[by], metrics.FLOW_BOUNDARIES[bx]

    def flow_stats(self, y_hat, y, u=0, v=1, dx=1.0, dy=1.0, boundary="auto", vort_hist=None, **norm):
        """Flow diagnostics of stored fields (lns_op_flow_stats): see metrics.flow_stats; boundary="auto" is resolved against
        this model.  The kernel body of rollout_eval_flow."""
        from . import metrics
        return metrics.flow_stats(y_hat, y, u=u, v=v, dx=dx, dy=dy, boundary=self._boundary_names(boundary), vort_hist=vort_hist, **norm)

    def vorticity(self, fields, u=0, v=1, dx=1.0, dy=1.0, boundary="auto", **norm):
        """The vorticity of stored fields [B,T,C,H,W] -> [B,T,H,W] (lns_op_vorticity): see metrics.vorticity."""
        from . import metrics
        return metrics.vorticity(fields, u=u, v=v, dx=dx, dy=dy, boundary=self._boundary_names(boundary), **norm)

    def _flow_select(self, fs, flow_steps, n_keep, stats_steps, hist, spectrum_steps, T, B, device, basis="dft"):
        """A `select` of _scored_call: the lns_eval_flow of the steps `flow_steps` under the lns_flow_spec fs, the vorticity of
        the n_keep kept frames, and the lns_eval_select of the (optional) statistics and spectra, or null."""
        import torch
        c = self.cfg
        sel = normalize_keep_steps(range(T) if flow_steps is None else flow_steps, T)
        arr = (ctypes.c_int * len(sel))(*sel)
        flow = torch.empty((B, len(sel), _lib.LNS_FLOW_STATS), dtype=torch.float32, device=device)
        counts = torch.empty((B, len(sel), 2, fs.nbins + 2), dtype=torch.int32, device=device) if fs.nbins else None
        vort = torch.empty((B, n_keep, c.Ly, c.Lx), dtype=torch.float32, device=device) if n_keep else None
        fl = _lib.LnsEvalFlow()
        fl.size = ctypes.sizeof(_lib.LnsEvalFlow)
        fl.n_flow, fl.flow_steps_host, fl.fspec = len(sel), arr, ctypes.pointer(fs)
        fl.flow_out, fl.hist_out, fl.vort_frames_out = flow.data_ptr(), self._ptr(counts), self._ptr(vort)
        q, stail = self._select_struct(stats_steps, hist, spectrum_steps, T, B, device, basis)
        qp = ctypes.byref(q) if (q.n_stats or q.n_spec) else None
        return (qp, ctypes.byref(fl)), (flow, counts, vort, sel) + stail, None

    def rollout_eval_flow(self, x, y, steps=None, param=None, keep_steps=(), flow_steps=None, u=0, v=1, dx=1.0, dy=1.0,
                          boundary="auto", vort_hist=None, vort_frames=True, stats_steps=(), hist=None, spectrum_steps=(),
                          spectrum_basis="dft", **norm):
        """rollout_eval with, for the steps `flow_steps` (what `normalize_keep_steps` takes; None: every step), the twelve flow
        diagnostics metrics.FLOW_STATS of the decoded frame against the truth across the velocity channels u (x-component) and
        v -- kinetic energy, enstrophy, rms divergence, vorticity error and cosine, velocity error, extrema -- with spacings
        dx / dy and `boundary` ("periodic", "wall", a pair (y, x) or "auto": periodic where this model's autoencoder pads
        circularly).  vort_hist = (nbins, lo, hi) adds the vorticity histograms of both; keep_steps with vort_frames adds the
        forecast's vorticity of the kept frames; `stats_steps` / `hist` and `spectrum_steps` (default: none) add
        rollout_eval_stats' statistics and rollout_eval_spectrum's spectra in the same pass.  Returns EvalFlow: flow / hist /
        vort_frames hold the bits of `flow_stats` / `vorticity` on rollout(x, T), every other field those of the existing
        calls.  The workspace is rollout_eval's."""
        fs = flow_spec(u, v, dx, dy, boundary, vort_hist, cfg=self.cfg)
        n_keep = len([int(s) for s in keep_steps]) if vort_frames else 0
        with self._spectrum_basis(spectrum_basis) as names:
            return self._scored_call("lns_rollout_eval_flow", EvalFlow, x, y, steps, None, param, keep_steps, norm,
                                     functools.partial(self._flow_select, fs, flow_steps, n_keep, stats_steps, hist, spectrum_steps,
                                                       basis=names))

    def rollout_latent_eval_flow(self, z, y, steps=None, t0=0, param=None, keep_steps=(), flow_steps=None, u=0, v=1, dx=1.0,
                                 dy=1.0, boundary="auto", vort_hist=None, vort_frames=True, stats_steps=(), hist=None,
                                 spectrum_steps=(), frame=None, seq=None, spectrum_basis="dft", **norm):
        """rollout_latent_eval with flow diagnostics: keep_steps, flow_steps, stats_steps and spectrum_steps are relative to the
        chunk, and flow / hist / vort_frames / stats / spectra belong to this chunk's steps.  Returns EvalFlowChunk (see
        rollout_latent_eval for frame / seq)."""
        fs = flow_spec(u, v, dx, dy, boundary, vort_hist, cfg=self.cfg)
        n_keep = len([int(s) for s in keep_steps]) if vort_frames else 0
        with self._spectrum_basis(spectrum_basis) as names:
            return self._scored_call("lns_rollout_latent_eval_flow", EvalFlowChunk, z, y, steps, t0, param, keep_steps, norm,
                                     functools.partial(self._flow_select, fs, flow_steps, n_keep, stats_steps, hist, spectrum_steps,
                                                       basis=names), frame, seq)

    # -- streaming validation with error attribution (include/lns.h "error attribution") ---------------------------
    def eval_attrib(self, y_hat, r, y, **norm):
        """The attribution columns of stored fields (lns_op_eval_attrib): see metrics.error_attribution.  The kernel bodies of
        rollout_eval_attrib."""
        from . import metrics
        return metrics.error_attribution(y_hat, r, y, **norm)

    def _attrib_select(self, return_latents, prev, B, T_total, device, frames):
        """The `attrib` of _scored_call: the lns_eval_attrib with every column set (prev: the previous chunk's result, whose
        tensors this chunk goes on filling) -> (the struct, EvalAttrib's fields after `frames`)."""
        import torch
        C = self.cfg.in_channels
        shapes = dict(recon_frame=(B, T_total, C), recon_seq=(B, C), prop_frame=(B, T_total, C), prop_seq=(B, C),
                      cross_frame=(B, T_total, C), cross_seq=(B, C), latent_frame=(B, T_total), latent_seq=(B,))
        if return_latents:
            shapes["z_true"] = (B, T_total) + self.latent_shape()
        t = {k: self._result(getattr(prev, k) if prev is not None else None, s, device) for k, s in shapes.items()}
        recon_frames = torch.empty_like(frames) if frames is not None else None
        at = _lib.LnsEvalAttrib()
        at.size = ctypes.sizeof(_lib.LnsEvalAttrib)
        for k in EvalAttrib._fields[3:11]:
            setattr(at, k, t[k].data_ptr())
        at.z_true_out = self._ptr(t.get("z_true"))
        at.recon_frames_out = self._ptr(recon_frames)
        return at, tuple(t[k] for k in EvalAttrib._fields[3:11]) + (recon_frames, t.get("z_true"))

    def rollout_eval_attrib(self, x, y, steps=None, param=None, keep_steps=(), return_latents=False, **norm):
        """rollout_eval with the rollout error of every plane split into the autoencoder's floor and the propagator's drift:
        beside the forecast of a decode group, the truth frames of the group are encoded and decoded again (r = D(E(y)), the
        reconstruction no propagator can beat) and the three fields are compared where they are decoded.  Returns EvalAttrib:
        frame / seq / frames hold rollout_eval's bits; recon_* those of `metrics.relative_l2(decode(encode(y)), y, ...)`;
        prop_* and cross_* those of `metrics.error_attribution` on the stored tensors, with frame^2 = prop^2 + recon^2 + cross
        (cross signed: > 0 the two errors add, < 0 they compensate; see metrics.attribution_shares); latent_* the relative L2
        of the propagated latent against encode(y_t); recon_frames the reconstructions of keep_steps; z_true (return_latents)
        encode(y).  Neither the rollout nor the reconstruction [B,T,C,Ly,Lx] is stored."""
        return self._scored_call("lns_rollout_eval_attrib", EvalAttrib, x, y, steps, None, param, keep_steps, norm,
                                 attrib=functools.partial(self._attrib_select, return_latents, None))

    def rollout_latent_eval_attrib(self, z, y, steps=None, t0=0, param=None, keep_steps=(), return_latents=False, prev=None, **norm):
        """rollout_latent_eval with error attribution.  The chunks of one horizon must follow each other on the same engine and
        batch; pass the previous chunk's result as `prev`: its tensors are filled further, and the chunk that completes the
        horizon writes every frame- and sequence-wise column.  keep_steps are relative to the chunk.  Returns EvalAttribChunk."""
        return self._scored_call("lns_rollout_latent_eval_attrib", EvalAttribChunk, z, y, steps, t0, param, keep_steps, norm,
                                 frame=prev.frame if prev is not None else None, seq=prev.seq if prev is not None else None,
                                 attrib=functools.partial(self._attrib_select, return_latents, prev))

    def autoencode_eval(self, x, param=None, return_latents=False, **norm):
        """The validation loop of the stage-1 scripts (train_stage1_ns2d.py:104-124) in one call: x [B,T,C,Ly,Lx] normalised ->
        AutoencodeEval(frame [B,T,C], seq [B,C], z [B,T,c,h,w] or None), the bits of
        `metrics.relative_l2(autoencoder(x), x, ...)` without the reconstruction being stored.  param [B]: a conditional
        encoder's, one value per trajectory.  Needs no propagator."""
        import torch
        x = self._dev(x)
        c = self.cfg
        if x.dim() != 5 or tuple(x.shape[2:]) != (c.in_channels, c.Ly, c.Lx):
            raise LnsError("autoencode_eval takes [B, T, %d, %d, %d], got %s" % (c.in_channels, c.Ly, c.Lx, tuple(x.shape)))
        B, T = int(x.shape[0]), int(x.shape[1])
        spec = eval_spec(c.in_channels, **norm)
        frame = torch.empty((B, T, c.in_channels), dtype=torch.float32, device=x.device)
        seq = torch.empty((B, c.in_channels), dtype=torch.float32, device=x.device)
        z = torch.empty((B, T) + self.latent_shape(), dtype=torch.float32, device=x.device) if return_latents else None
        p = self._param(param, x)
        with torch.cuda.device(x.device):
            ws = self._sized_workspace("lns_autoencode_eval_workspace_bytes", B, x.device)
            self._check(self._L.lns_autoencode_eval(self._h, x.data_ptr(), self._ptr(p), B, T, ctypes.byref(spec), frame.data_ptr(),
                                                    seq.data_ptr(), self._ptr(z), ws.data_ptr(), ws.numel(), self._stream(x)),
                        "lns_autoencode_eval")
        return AutoencodeEval(frame, seq, z)

    # -- training rollout of the propagator (include/lns.h "training rollout") ------------------------------------
    def _ptr_array(self, tensors):
        """ctypes array of device pointers in parameter-table order; tensors: {key: fp32 contiguous device tensor}."""
        arr = (ctypes.c_void_p * len(self.params))()
        for i, (key, shape, _) in enumerate(self.params):
            t = tensors.get(key)
            if t is None:
                arr[i] = None
                continue
            if not t.is_cuda or t.dtype is not __import__("torch").float32 or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
                raise LnsError("training rollout: %s must be a contiguous fp32 device tensor of shape %s" % (key, tuple(shape)))
            arr[i] = t.data_ptr()
        return arr

    def train_forward(self, params, z_in, T, param=None, workspace=None):
        """z_pred [B,T,c,h,w] of the latent rollout started at z_in [B,c,h,w], with the tape kept for train_backward.
        params: {state_dict key: device tensor} of (at least) the propagator's parameters, or the pointer array
        `_ptr_array` returns; param: [B] (conditional).  workspace: the caller's (train_tangent needs the larger one of
        train_tangent_workspace_bytes); None: one of lns_train_workspace_bytes is allocated."""
        import torch
        z_in = self._dev(z_in)
        pc = self._param(param, z_in)
        B, c, h, w = z_in.shape
        ws = workspace
        if ws is None:
            n = ctypes.c_size_t(0)
            self._check(self._L.lns_train_workspace_bytes(self._h, B, h, w, int(T), ctypes.byref(n)), "lns_train_workspace_bytes")
            ws = torch.empty(int(n.value), dtype=torch.uint8, device=z_in.device)
        z_pred = torch.empty((B, int(T), c, h, w), dtype=torch.float32, device=z_in.device)
        self._check(self._L.lns_train_forward(self._h, self._ptr_array(params) if isinstance(params, dict) else params, z_in.data_ptr(),
                                              pc.data_ptr() if pc is not None else None, B, h, w, int(T), z_pred.data_ptr(),
                                              ws.data_ptr(), ws.numel(), self._stream(z_in)), "lns_train_forward")
        return z_pred, ws

    def train_backward(self, params, z_in, z_pred, grad_z_pred, ws, need_z_grad=False, need_param_grad=False, state_only=False):
        """{key: gradient tensor} of every propagator parameter (+ grad of z_in if asked) for dL/dz_pred.
        need_param_grad (conditional propagator): a third result, d loss / d param [B].  state_only: the state-only adjoint
        (lns_train_backward_ex with no gradient array) -- no parameter gradient is computed, the first result is {}."""
        import torch
        z_in = self._dev(z_in)
        g = self._dev(grad_z_pred)
        B, T, c, h, w = z_pred.shape
        prefix = self.cfg.prop_prefix.decode()
        grads = {} if state_only else {k: torch.empty(tuple(shp), dtype=torch.float32, device=z_in.device)
                                       for k, shp, _ in self.params if k.startswith(prefix)}
        gz = torch.empty_like(z_in) if need_z_grad else None
        if not need_param_grad and not state_only:
            self._check(self._L.lns_train_backward(self._h, self._ptr_array(params), z_in.data_ptr(), z_pred.data_ptr(), g.data_ptr(),
                                                   B, h, w, T, self._ptr_array(grads), gz.data_ptr() if gz is not None else None,
                                                   ws.data_ptr(), ws.numel(), self._stream(z_in)), "lns_train_backward")
            return grads, gz
        gp = torch.empty(B, dtype=torch.float32, device=z_in.device) if need_param_grad else None
        self._check(self._L.lns_train_backward_ex(self._h, self._ptr_array(params), z_in.data_ptr(), z_pred.data_ptr(), g.data_ptr(),
                                                  B, h, w, T, None if state_only else self._ptr_array(grads), self._ptr(gz),
                                                  ws.data_ptr(), ws.numel(), self._stream(z_in), self._ptr(gp)),
                    "lns_train_backward_ex")
        return (grads, gz, gp) if need_param_grad else (grads, gz)

    # -- tangent-linear rollout (include/lns.h "tangent-linear rollout") ---------------------------------------------
    orthonormalize = staticmethod(orthonormalize)

    def train_tangent_workspace_bytes(self, B, h, w, T, K):
        """Bytes of the workspace train_forward(..., workspace=) and train_tangent share for K tangents per sample: the
        training workspace under the current "train_wgrad" plus the tangent scratch.  Needs no GPU."""
        n = ctypes.c_size_t(0)
        self._check(self._L.lns_train_tangent_workspace_bytes(self._h, int(B), int(h), int(w), int(T), int(K), ctypes.byref(n)),
                    "lns_train_tangent_workspace_bytes")
        return int(n.value)

    def train_tangent(self, params, v, T, workspace, t0=0, nsteps=None, keep=False, jv_out=None):
        """J v along the trajectory of the train_forward(..., T, workspace=workspace) that precedes this call: v [B,K,c,h,w]
        (K tangents of every sample's latent before step t0) is advanced IN PLACE through the steps t0 .. t0 + nsteps - 1
        (nsteps None: to T).  keep / jv_out: also the tangents after every one of those steps, [B,K,nsteps,c,h,w]
        (returned; None otherwise).  params as in train_forward.  Never synchronises; allocates only jv_out under keep."""
        import torch
        if not isinstance(v, torch.Tensor) or not v.is_cuda or v.dtype != torch.float32 or v.dim() != 5 or not v.is_contiguous():
            raise LnsError("train_tangent advances v in place: a contiguous fp32 [B,K,c,h,w] HIP device tensor, got %s"
                           % (tuple(v.shape) if isinstance(v, torch.Tensor) else type(v),))
        B, K, c, h, w = v.shape
        nsteps = int(T) - int(t0) if nsteps is None else int(nsteps)
        if keep and jv_out is None:
            jv_out = torch.empty((B, K, max(nsteps, 0), c, h, w), dtype=torch.float32, device=v.device)
        if jv_out is not None and (tuple(jv_out.shape) != (B, K, nsteps, c, h, w) or jv_out.dtype != torch.float32
                                   or not jv_out.is_contiguous() or jv_out.device != v.device):
            raise LnsError("jv_out must be a contiguous fp32 [B,K,nsteps,c,h,w] tensor on v's device")
        with torch.cuda.device(v.device):
            self._check(self._L.lns_train_tangent(self._h, self._ptr_array(params) if isinstance(params, dict) else params, B, h, w,
                                                  int(T), K, int(t0), nsteps, v.data_ptr(), self._ptr(jv_out), workspace.data_ptr(),
                                                  workspace.numel(), self._stream(v)), "lns_train_tangent")
        return jv_out

    # -- latent fit (include/lns.h "latent fit") ---------------------------------------------------------------------
    obs_loss = staticmethod(obs_loss)

    def fit_step_workspace_bytes(self, B, h, w, T, n_obs):
        """Bytes of the workspace of fit_step for T = last observed step + 1 rollout steps and n_obs observations."""
        n = ctypes.c_size_t(0)
        self._check(self._L.lns_fit_step_workspace_bytes(self._h, int(B), int(h), int(w), int(T), int(n_obs), ctypes.byref(n)),
                    "lns_fit_step_workspace_bytes")
        return int(n.value)

    def fit_step(self, params, z0, obs, spec, param=None, z_background=None, g_z=None, exp_avg_z=None, exp_avg_sq_z=None, g_p=None,
                 exp_avg_p=None, exp_avg_sq_p=None, loss=None, per=None, workspace=None):
        """One iteration of fitting z0 [B,c,h,w] and / or param [B] to the observed latents obs [B,n_obs,c,h,w]
        (lns_fit_step): training forward, observation loss, state-only adjoint, Adam -- z0 / param are updated IN PLACE.
        spec: fit_spec(...).  params: {key: tensor} or the pointer array `_ptr_array` returns.  g_* / exp_avg_*: the caller's
        gradient buffers and Adam moments of what is fitted.  Returns (loss [B] before the update, per [B,n_obs]); nothing
        here synchronises, and with loss / per / workspace given nothing allocates."""
        import torch
        for t_, name in ((z0, "z0"), (param, "param")):
            if isinstance(t_, torch.Tensor) and not t_.is_contiguous():
                raise LnsError("fit_step updates %s in place: it must be contiguous" % name)
        z0, obs = self._dev(z0), self._dev(obs)
        B, c, h, w = z0.shape
        if obs.dim() != 5 or obs.shape[0] != B or obs.shape[1] != spec.n_obs or tuple(obs.shape[2:]) != (c, h, w) or obs.device != z0.device:
            raise LnsError("obs must be [B,%d,%d,%d,%d] on z0's device, got %s on %s" % (spec.n_obs, c, h, w, tuple(obs.shape), obs.device))
        if param is not None:
            param = self._dev(param)
            if tuple(param.shape) != (B,) or param.device != z0.device:
                raise LnsError("param must be [B] on z0's device")
        if z_background is not None:
            z_background = self._dev(z_background)
            if z_background.shape != z0.shape or z_background.device != z0.device:
                raise LnsError("z_background must match z0")
        for t_, like, name in ((g_z, z0, "g_z"), (exp_avg_z, z0, "exp_avg_z"), (exp_avg_sq_z, z0, "exp_avg_sq_z"), (g_p, param, "g_p"),
                               (exp_avg_p, param, "exp_avg_p"), (exp_avg_sq_p, param, "exp_avg_sq_p")):
            if t_ is not None and (like is None or t_.shape != like.shape or t_.device != z0.device or t_.dtype != torch.float32
                                   or not t_.is_contiguous()):
                raise LnsError("%s must be a contiguous fp32 tensor like what it belongs to" % name)
        T = int(spec._steps[spec.n_obs - 1]) + 1
        with torch.cuda.device(z0.device):
            if workspace is None:
                workspace = torch.empty(self.fit_step_workspace_bytes(B, h, w, T, spec.n_obs), dtype=torch.uint8, device=z0.device)
            if loss is None:
                loss = torch.empty(B, dtype=torch.float32, device=z0.device)
            if per is None:
                per = torch.empty((B, spec.n_obs), dtype=torch.float32, device=z0.device)
            self._check(self._L.lns_fit_step(self._h, self._ptr_array(params) if isinstance(params, dict) else params, z0.data_ptr(),
                                             self._ptr(param), obs.data_ptr(), self._ptr(z_background), B, h, w, ctypes.byref(spec),
                                             self._ptr(g_z), self._ptr(exp_avg_z), self._ptr(exp_avg_sq_z), self._ptr(g_p),
                                             self._ptr(exp_avg_p), self._ptr(exp_avg_sq_p), loss.data_ptr(), per.data_ptr(),
                                             workspace.data_ptr(), workspace.numel(), self._stream(z0)), "lns_fit_step")
        return loss, per

    # -- latent fit: Gauss-Newton (include/lns.h "latent fit: Gauss-Newton") ------------------------------------------
    cg_start = staticmethod(cg_start)
    cg_update = staticmethod(cg_update)

    def train_gn_product_workspace_bytes(self, B, h, w, T, n_obs):
        """Bytes of the workspace train_forward(..., workspace=) and train_gn_product share: train_tangent's for K = 1 plus the
        cotangent and the double partials.  Needs no GPU."""
        n = ctypes.c_size_t(0)
        self._check(self._L.lns_train_gn_product_workspace_bytes(self._h, int(B), int(h), int(w), int(T), int(n_obs), ctypes.byref(n)),
                    "lns_train_gn_product_workspace_bytes")
        return int(n.value)

    def train_gn_product(self, params, z_in, z_pred, v, obs_steps, workspace, weights=None, background=0.0, damping=0.0, hv=None,
                         vhv=None, need_vhv=True):
        """(H v, v^T H v) of the Gauss-Newton operator of the observation loss at z_in, on the tape of the
        train_forward(params, z_in, T = obs_steps[-1] + 1, workspace=workspace) that gave z_pred: v [B,c,h,w] is only read;
        hv like v and vhv [B] float64 are the caller's or allocated (need_vhv False and vhv None: no vhv).  Never
        synchronises; with hv / vhv given nothing allocates."""
        import torch
        z_in, v = self._dev(z_in), self._dev(v)
        steps, w_ = normalize_obs(obs_steps, weights)
        B, c, h, w = z_in.shape
        T = steps[-1] + 1
        if v.shape != z_in.shape or v.device != z_in.device:
            raise LnsError("v must be [B,c,h,w] like z_in %s on its device, got %s" % (tuple(z_in.shape), tuple(v.shape)))
        if tuple(z_pred.shape) != (B, T, c, h, w) or z_pred.dtype != torch.float32 or not z_pred.is_contiguous() or z_pred.device != z_in.device:
            raise LnsError("z_pred must be the contiguous fp32 [B,%d,c,h,w] of the forward over the last observed step + 1" % T)
        with torch.cuda.device(z_in.device):
            if hv is None:
                hv = torch.empty_like(v)
            if vhv is None and need_vhv:
                vhv = torch.empty(B, dtype=torch.float64, device=z_in.device)
            if hv.shape != v.shape or hv.dtype != torch.float32 or not hv.is_contiguous() or hv.device != v.device:
                raise LnsError("hv must be a contiguous fp32 tensor like v")
            if vhv is not None and (tuple(vhv.shape) != (B,) or vhv.dtype != torch.float64 or not vhv.is_contiguous() or vhv.device != v.device):
                raise LnsError("vhv must be a contiguous float64 [B] tensor on v's device")
            self._check(self._L.lns_train_gn_product(
                self._h, self._ptr_array(params) if isinstance(params, dict) else params, z_in.data_ptr(), z_pred.data_ptr(), B, h, w, T,
                len(steps), (ctypes.c_int * len(steps))(*steps), (ctypes.c_double * len(w_))(*w_), float(background), float(damping),
                v.data_ptr(), hv.data_ptr(), self._ptr(vhv), workspace.data_ptr(), workspace.numel(), self._stream(z_in)),
                "lns_train_gn_product")
        return hv, vhv

    def fit_gn_step_workspace_bytes(self, B, h, w, T, n_obs):
        """Bytes of the workspace of fit_gn_step for T = last observed step + 1 rollout steps and n_obs observations."""
        n = ctypes.c_size_t(0)
        self._check(self._L.lns_fit_gn_step_workspace_bytes(self._h, int(B), int(h), int(w), int(T), int(n_obs), ctypes.byref(n)),
                    "lns_fit_gn_step_workspace_bytes")
        return int(n.value)

    def fit_gn_step(self, params, z0, obs, spec, param=None, z_background=None, loss=None, per=None, cg_resid=None, applied=None,
                    workspace=None):
        """One outer Gauss-Newton iteration on z0 [B,c,h,w], IN PLACE (lns_fit_gn_step): training forward, observation loss,
        state-only adjoint, spec.n_cg steps of conjugate gradients on H delta = -g with H v from the tangent and the adjoint,
        z0 += delta.  spec: gn_spec(...); param [B]: the conditional propagator's known input.  Returns (loss [B] before the
        update, per [B,n_obs], cg_resid [B] = |r| / |r0|, applied [B] int32); nothing here synchronises, and with the four
        outputs and the workspace given nothing allocates."""
        import torch
        if isinstance(z0, torch.Tensor) and not z0.is_contiguous():
            raise LnsError("fit_gn_step updates z0 in place: it must be contiguous")
        z0, obs = self._dev(z0), self._dev(obs)
        B, c, h, w = z0.shape
        if obs.dim() != 5 or obs.shape[0] != B or obs.shape[1] != spec.n_obs or tuple(obs.shape[2:]) != (c, h, w) or obs.device != z0.device:
            raise LnsError("obs must be [B,%d,%d,%d,%d] on z0's device, got %s on %s" % (spec.n_obs, c, h, w, tuple(obs.shape), obs.device))
        if param is not None:
            param = self._dev(param)
            if tuple(param.shape) != (B,) or param.device != z0.device:
                raise LnsError("param must be [B] on z0's device")
        if z_background is not None:
            z_background = self._dev(z_background)
            if z_background.shape != z0.shape or z_background.device != z0.device:
                raise LnsError("z_background must match z0")
        T = int(spec._steps[spec.n_obs - 1]) + 1
        with torch.cuda.device(z0.device):
            dev = z0.device
            if workspace is None:
                workspace = torch.empty(self.fit_gn_step_workspace_bytes(B, h, w, T, spec.n_obs), dtype=torch.uint8, device=dev)
            loss = torch.empty(B, dtype=torch.float32, device=dev) if loss is None else loss
            per = torch.empty((B, spec.n_obs), dtype=torch.float32, device=dev) if per is None else per
            cg_resid = torch.empty(B, dtype=torch.float32, device=dev) if cg_resid is None else cg_resid
            applied = torch.empty(B, dtype=torch.int32, device=dev) if applied is None else applied
            for t_, shape, dt, name in ((loss, (B,), torch.float32, "loss"), (per, (B, spec.n_obs), torch.float32, "per"),
                                        (cg_resid, (B,), torch.float32, "cg_resid"), (applied, (B,), torch.int32, "applied")):
                if tuple(t_.shape) != shape or t_.dtype != dt or not t_.is_contiguous() or t_.device != dev:
                    raise LnsError("%s must be a contiguous %s tensor of shape %s on z0's device" % (name, dt, shape))
            self._check(self._L.lns_fit_gn_step(self._h, self._ptr_array(params) if isinstance(params, dict) else params, z0.data_ptr(),
                                                self._ptr(param), obs.data_ptr(), self._ptr(z_background), B, h, w, ctypes.byref(spec),
                                                loss.data_ptr(), per.data_ptr(), cg_resid.data_ptr(), applied.data_ptr(),
                                                workspace.data_ptr(), workspace.numel(), self._stream(z0)), "lns_fit_gn_step")
        return loss, per, cg_resid, applied

    # -- device-resident training step (include/lns.h "device-resident training step") -------------------------------
    smooth_l1 = staticmethod(smooth_l1)

    def adam_step(self, params, grads, exp_avg, exp_avg_sq, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, step=1):
        """torch.optim.Adam's update of every tensor present in all four {key: device tensor} dicts, in one launch
        (lns_adam_step).  step: 1-based count of this update.  In place; the caller bumps the tensors' versions."""
        import torch
        spec = adam_spec(lr, betas, eps, weight_decay, step)
        any_t = next(iter(params.values()))
        with torch.cuda.device(any_t.device):
            self._check(self._L.lns_adam_step(self._h, self._ptr_array(params), self._ptr_array(grads), self._ptr_array(exp_avg),
                                              self._ptr_array(exp_avg_sq), ctypes.byref(spec), self._stream(any_t)), "lns_adam_step")

    def conv_wgrad(self, dy, x, ksize, dilation=1, pad_y=LNS_PAD_CIRCULAR, pad_x=LNS_PAD_CIRCULAR, form=1, accumulate=False, dw=None):
        """Weight gradient of a stride-1 "same" convolution (lns_op_conv_wgrad): dy [B,Cout,H,W], x [B,Cin,H,W] ->
        dw [Cout,Cin,ksize,ksize].  form 0: one block per output tile; 1: batch-parallel (option "train_wgrad").
        accumulate: added to the given dw.  Synchronises."""
        import torch
        dy, x = self._dev(dy), self._dev(x)
        B, Cout, H, W = dy.shape
        Cin = x.shape[1]
        if x.dim() != 4 or (x.shape[0], x.shape[2], x.shape[3]) != (B, H, W) or x.device != dy.device:
            raise LnsError("conv_wgrad: x must be [B,Cin,%d,%d] on dy's device, got %s on %s" % (H, W, tuple(x.shape), x.device))
        if dw is None:
            if accumulate:
                raise LnsError("conv_wgrad: accumulate needs dw")
            dw = torch.empty((Cout, Cin, ksize, ksize), dtype=torch.float32, device=dy.device)
        elif tuple(dw.shape) != (Cout, Cin, ksize, ksize) or dw.dtype != torch.float32 or not dw.is_contiguous() or dw.device != dy.device:
            raise LnsError("conv_wgrad: dw must be a contiguous fp32 [%d,%d,%d,%d] tensor on dy's device" % (Cout, Cin, ksize, ksize))
        n = ctypes.c_size_t(0)
        rc = self._L.lns_op_conv_wgrad_scratch_bytes(B, Cin, Cout, H, W, int(ksize), int(form), ctypes.byref(n))
        with torch.cuda.device(dy.device):
            scratch = torch.empty(max(int(n.value), 4), dtype=torch.uint8, device=dy.device) if rc == 0 else None
            if rc == 0:
                rc = self._L.lns_op_conv_wgrad(dy.data_ptr(), x.data_ptr(), B, Cin, Cout, H, W, int(ksize), int(dilation), int(pad_y),
                                               int(pad_x), int(form), int(bool(accumulate)), dw.data_ptr(), scratch.data_ptr(),
                                               int(n.value), self._stream(dy))
        _op_check(rc, "lns_op_conv_wgrad")
        return dw

    def train_step_workspace_bytes(self, B, h, w, T):
        """Bytes of the workspace of train_step; follows the "train_wgrad" option (set_option)."""
        n = ctypes.c_size_t(0)
        self._check(self._L.lns_train_step_workspace_bytes(self._h, int(B), int(h), int(w), int(T), ctypes.byref(n)),
                    "lns_train_step_workspace_bytes")
        return int(n.value)

    def train_step(self, params, z_in, z_out, grads, param=None, beta=1.0, exp_avg=None, exp_avg_sq=None, spec=None,
                   loss_out=None, workspace=None):
        """One stage-2 training step on the device (lns_train_step): training forward from z_in [B,1,c,h,w] (or [B,c,h,w]),
        smooth-L1 loss against z_out [B,T,c,h,w], backward through time into `grads`, and -- with `spec` (adam_spec(...)) --
        Adam on params / exp_avg / exp_avg_sq.  params & co.: {key: tensor} dicts, or ctypes pointer arrays in table order
        (what `_ptr_array` returns; `lns_amd.train.Stage2Trainer` resolves them once).  Returns the 0-dim device loss
        (before the update).  Nothing here synchronises; with `loss_out` and `workspace` given nothing allocates."""
        import torch
        z_in, z_out = self._dev(z_in), self._dev(z_out)
        if z_in.dim() == 5:
            if z_in.shape[1] != 1:
                raise LnsError("z_in must be [B,1,c,h,w] (t_in == 1)")
            z_in = z_in[:, 0]
        B, c, h, w = z_in.shape
        if z_out.dim() != 5 or z_out.shape[0] != B or tuple(z_out.shape[2:]) != (c, h, w) or z_out.device != z_in.device:
            raise LnsError("z_out must be [B,T,%d,%d,%d] on z_in's device, got %s on %s" % (c, h, w, tuple(z_out.shape), z_out.device))
        T = int(z_out.shape[1])
        pc = self._param(param, z_in)

        def arr(t):
            return self._ptr_array(t) if isinstance(t, dict) else t
        with torch.cuda.device(z_in.device):
            if workspace is None:
                workspace = torch.empty(self.train_step_workspace_bytes(B, h, w, T), dtype=torch.uint8, device=z_in.device)
            if loss_out is None:
                loss_out = torch.empty((), dtype=torch.float32, device=z_in.device)
            self._check(self._L.lns_train_step(self._h, arr(params), z_in.data_ptr(), z_out.data_ptr(),
                                               pc.data_ptr() if pc is not None else None, B, h, w, T, float(beta), arr(grads),
                                               arr(exp_avg) if exp_avg is not None else None,
                                               arr(exp_avg_sq) if exp_avg_sq is not None else None,
                                               _ref(spec), loss_out.data_ptr(), workspace.data_ptr(), workspace.numel(),
                                               self._stream(z_in)), "lns_train_step")
        return loss_out

    def train_step_clip_workspace_bytes(self, B, h, w, T):
        """Bytes of the workspace of train_step_clip: train_step's, then the norm partials, the clip coefficient (768 bytes
        before the end), the norm and the counter of skipped steps (256 bytes before the end; the caller zeroes it once)."""
        n = ctypes.c_size_t(0)
        self._check(self._L.lns_train_step_clip_workspace_bytes(self._h, int(B), int(h), int(w), int(T), ctypes.byref(n)),
                    "lns_train_step_clip_workspace_bytes")
        return int(n.value)

    def train_step_clip(self, params, z_in, z_out, grads, exp_avg, exp_avg_sq, spec, param=None, beta=1.0, loss_out=None,
                        norm_out=None, workspace=None):
        """train_step with gradient-norm clipping and / or AdamW (lns_train_step_clip): forward, loss, backward, the global
        L2 norm of the propagator's gradients, then the update on the clipped gradients, which `grads` hold afterwards.
        spec: update_spec(...).  Returns (loss, norm before clipping) as 0-dim device tensors; never synchronises.  A
        workspace allocated here has its counter of skipped steps zeroed; a caller's own workspace is the caller's to zero."""
        import torch
        z_in, z_out = self._dev(z_in), self._dev(z_out)
        if z_in.dim() == 5:
            if z_in.shape[1] != 1:
                raise LnsError("z_in must be [B,1,c,h,w] (t_in == 1)")
            z_in = z_in[:, 0]
        B, c, h, w = z_in.shape
        if z_out.dim() != 5 or z_out.shape[0] != B or tuple(z_out.shape[2:]) != (c, h, w) or z_out.device != z_in.device:
            raise LnsError("z_out must be [B,T,%d,%d,%d] on z_in's device, got %s on %s" % (c, h, w, tuple(z_out.shape), z_out.device))
        T = int(z_out.shape[1])
        pc = self._param(param, z_in)

        def arr(t):
            return self._ptr_array(t) if isinstance(t, dict) else t
        with torch.cuda.device(z_in.device):
            if workspace is None:
                workspace = torch.empty(self.train_step_clip_workspace_bytes(B, h, w, T), dtype=torch.uint8, device=z_in.device)
                workspace[-256:].zero_()
            if loss_out is None:
                loss_out = torch.empty((), dtype=torch.float32, device=z_in.device)
            if norm_out is None:
                norm_out = torch.empty((), dtype=torch.float32, device=z_in.device)
            self._check(self._L.lns_train_step_clip(self._h, arr(params), z_in.data_ptr(), z_out.data_ptr(),
                                                    pc.data_ptr() if pc is not None else None, B, h, w, T, float(beta), arr(grads),
                                                    arr(exp_avg), arr(exp_avg_sq), ctypes.byref(spec), loss_out.data_ptr(),
                                                    norm_out.data_ptr(), workspace.data_ptr(), workspace.numel(),
                                                    self._stream(z_in)), "lns_train_step_clip")
        return loss_out, norm_out

    def check_finite(self, B, device=None):
        """Raises LnsError naming the first layer / sample whose output held inf or NaN in the LAST call (encode /
        decode / propagate / rollout) for batch B.  Coverage: every tensor a layer of that call wrote, including
        the plan outputs; for a rollout the amax records are per plan RUN, so what is seen is the last propagator
        step and the last decode on each decode stream -- `set_option("track_nonfinite", 1)` adds a sticky word that
        also remembers the earlier steps / decode groups (one tiny extra launch per plan run).
        Synchronises the device's current stream; reads a few KB of the workspace back."""
        import torch
        dev = torch.device("cuda" if device is None else device)
        if dev.type != "cuda":
            raise LnsError("check_finite: %s is not a HIP device" % (dev,))
        dev = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
        ws = self._ws.get((B, dev))
        if ws is None:
            raise LnsError("no run for batch %d on %s yet" % (B, dev))
        stream = ctypes.c_void_p(torch.cuda.current_stream(ws.device).cuda_stream)
        self._check(self._L.lns_check_finite(self._h, int(B), ws.data_ptr(), ws.numel(), stream), "lns_check_finite")

    # -- diagnostics ----------------------------------------------------------------
    def trace_enable(self, on=True):
        self._check(self._L.lns_trace_enable(self._h, int(on)), "lns_trace_enable")

    def trace(self):
        out = []
        name = ctypes.create_string_buffer(_lib_key_cap())
        shp = (ctypes.c_int64 * 4)()
        for i in range(self._L.lns_trace_count(self._h)):
            self._check(self._L.lns_trace_info(self._h, i, name, len(name), shp), "lns_trace_info")
            a = np.empty(tuple(int(s) for s in shp), np.float32)
            self._check(self._L.lns_trace_copy(self._h, i, a.ctypes.data_as(ctypes.c_void_p)), "lns_trace_copy")
            out.append((name.value.decode(), a))
        return out

    def timing_enable(self, on=True):
        self._check(self._L.lns_timing_enable(self._h, int(on)), "lns_timing_enable")

    def timing_event_overhead_us(self):
        """Per-launch overhead the engine measured for its HIP-event timing and subtracted from every timed launch."""
        v = ctypes.c_double()
        try:
            self._check(self._L.lns_timing_mfma_flops(self._h, -1, ctypes.byref(v)), "lns_timing_mfma_flops")
        except _lib.LnsLibraryError:
            return None
        return v.value if v.value >= 0 else None

    def timing(self):
        out = {}
        name = ctypes.create_string_buffer(_lib_key_cap())
        ms, fl, by = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        n = ctypes.c_int64()
        for i in range(self._L.lns_timing_count(self._h)):
            self._check(self._L.lns_timing_info(self._h, i, name, len(name), ctypes.byref(ms), ctypes.byref(n),
                                                ctypes.byref(fl), ctypes.byref(by)), "lns_timing_info")
            mf = ctypes.c_double()
            try:
                self._check(self._L.lns_timing_mfma_flops(self._h, i, ctypes.byref(mf)), "lns_timing_mfma_flops")
            except _lib.LnsLibraryError:      # an earlier round's build under LNS_HIP_LIB (A/B runs): no executed-FLOP records
                pass
            if n.value:
                out[name.value.decode()] = dict(ms=ms.value, launches=int(n.value), flops=fl.value, bytes=by.value,
                                                mfma_flops=mf.value)
        return out


def _lib_key_cap():
    return 160


def param_shapes(args, **kw):
    """{state_dict key: shape} of the model `args` describes (no GPU needed)."""
    return Engine(make_config(args, **kw)).param_shapes()

"""Drop-in `nn.Module` surface of the hot path.

The classes here keep the reference's constructor arguments, method names,
attribute names and state_dict keys/shapes
    SimpleAutoencoder(args).encode/decode/forward/load_checkpoint   modules/autoencoder2d.py:160-186
    SimpleCNN(latent_dim, [cond_emb_dim,] prop_n_block, prop_n_embd, dilation)(z[, param])
                                                                   train_stage2_ns2d.py:56-87
    LatentDynamics(args).x_to_z/z_to_x/predict/load_autoencoder     train_stage2_ns2d.py:90-158
but hold NO arithmetic: the parameter tree is generated from the engine's
parameter table (the single definition of the architecture lives in
csrc/lns_model.cpp) and every call runs the HIP engine through the C ABI.
Gradients exist through ONE entry point, `LatentDynamics.forward(z_in, z_out[, param], loss_fn)` (the stage-2 training
rollout), and only for the propagator's parameters.  Everything else is inference (the reference wraps this
path in torch.no_grad()): autoencoder parameters are created with requires_grad=False (stage-1 training is out of scope),
and `SimpleCNN.forward` / `SimpleAutoencoder.{encode,decode,forward}` raise LnsError when they are called with autograd
enabled on something that requires grad -- instead of returning a tensor without grad_fn that only fails at backward().
"""
import math
import types

import numpy as np
import torch
import torch.nn as nn

from . import engine as _engine
from ._lib import (LNS_AE_HALF_PERIODIC, LNS_AE_NONE, LNS_AE_NONSQUARED, LNS_AE_SQUARE,
                   LNS_PAD_CIRCULAR, LNS_PAD_ZEROS, LNS_PROP_CONDITIONAL, LNS_PROP_NONE,
                   LNS_PROP_PLAIN, LnsError)


# Bumped whenever a drop-in module's parameter TREE may have changed identity: a Parameter / buffer object replaced
# (`mod.x.weight = nn.Parameter(...)`, `load_state_dict(assign=True)`, `.to()` / `.cuda()` / `.float()`, which always
# rebind buffers).  `_Hosted._engine` caches the flat (key, tensor) list and re-walks the tree when the epoch moved;
# in-place changes (optimizer steps, `load_state_dict`, `copy_`) are caught by (storage pointer, version) per tensor.
_TREE_EPOCH = [0]


class _TreeWatch(nn.Module):
    """Mix-in of every drop-in module: any rebinding of a tensor / sub-module invalidates the cached flat list."""

    def __setattr__(self, name, value):
        if isinstance(value, (torch.Tensor, nn.Module)) or name in self.__dict__.get("_parameters", ()) or \
                name in self.__dict__.get("_buffers", ()):
            _TREE_EPOCH[0] += 1
        super().__setattr__(name, value)

    def __delattr__(self, name):
        _TREE_EPOCH[0] += 1
        super().__delattr__(name)

    def register_parameter(self, name, param):
        _TREE_EPOCH[0] += 1
        super().register_parameter(name, param)

    def register_buffer(self, name, tensor, persistent=True):
        _TREE_EPOCH[0] += 1
        super().register_buffer(name, tensor, persistent=persistent)

    def _apply(self, fn, *a, **k):
        _TREE_EPOCH[0] += 1
        r = super()._apply(fn, *a, **k)
        _TREE_EPOCH[0] += 1
        return r

    def load_state_dict(self, *a, **k):
        _TREE_EPOCH[0] += 1
        r = super().load_state_dict(*a, **k)
        _TREE_EPOCH[0] += 1
        return r

    def _load_from_state_dict(self, *a, **k):      # the per-module step of a PARENT's load_state_dict(assign=True)
        super()._load_from_state_dict(*a, **k)
        _TREE_EPOCH[0] += 1


class _Node(_TreeWatch):
    """Parameter container mirroring one reference sub-module."""

    def forward(self, *a, **k):
        raise LnsError("sub-modules of the drop-in hold parameters only; call the owning "
                       "SimpleAutoencoder / SimpleCNN / LatentDynamics")


def _init_value(key, shape, sibling_weight_shape):
    """PyTorch-default-like initial values (reference constructors rely on
    nn.Conv2d/nn.Linear defaults, SABlock._init_weights basics.py:358-369,
    zero_module cond_utils.py:12-16, spectral weights basics.py:119-124)."""
    leaf = key.rsplit(".", 1)[-1]
    t = torch.empty(shape, dtype=torch.float32)
    sa = any(s in key for s in (".to_q.", ".to_k.", ".to_v.", ".proj_out."))
    zero = (".cond_conv1.2." in key) or (".cond_conv2.3." in key) or \
        (key.startswith("encoder.") and ".conv2." in key and (".layers." in key or ".to_out_conv." in key))   # zero_module (cond_utils.py:96-97)
    if leaf == "inv_freq":
        dim = 2 * shape[0]
        return 1.0 / (10000 ** (torch.arange(0, dim, 2).float() / dim))
    if zero:
        return t.zero_()
    if leaf == "pe":
        return t.normal_(0.0, 0.02)
    if leaf in ("weights1", "weights2") and len(shape) == 5:
        return t.uniform_(0, 1).mul_(1.0 / (shape[0] * shape[1]))
    if len(shape) >= 2:
        if sa:
            return t.normal_(0.0, 0.02)
        fan_in = int(np.prod(shape[1:]))
        b = 1.0 / math.sqrt(fan_in)
        return t.uniform_(-b, b)
    if leaf == "weight":
        return t.fill_(1.0)
    if sibling_weight_shape is not None and len(sibling_weight_shape) >= 2 and not sa:
        b = 1.0 / math.sqrt(int(np.prod(sibling_weight_shape[1:])))
        return t.uniform_(-b, b)
    return t.zero_()


def _no_backward(what, *tensors, params=()):
    """Called at the top of an inference-only forward.  With autograd enabled and an input (or a parameter) that requires
    grad the caller expects a differentiable result; there is no backward for this path, so say so here."""
    if not torch.is_grad_enabled():
        return
    if any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors) or any(p.requires_grad for p in params):
        raise LnsError("%s has no backward: gradients exist only through LatentDynamics.forward(z_in, z_out[, param], "
                       "loss_fn); call it under torch.no_grad() (or on tensors / parameters with requires_grad=False)" % what)


def _grow_tree(root, table, strip="", requires_grad=True):
    shapes = {k: s for k, s, _ in table}
    for key, shape, is_buffer in table:
        assert key.startswith(strip), (key, strip)
        parts = key[len(strip):].split(".")
        node = root
        for p in parts[:-1]:
            if not hasattr(node, p):
                node.add_module(p, _Node())
            node = getattr(node, p)
        sib = shapes.get(key.rsplit(".", 1)[0] + ".weight")
        val = _init_value(key, shape, sib)
        if is_buffer:
            node.register_buffer(parts[-1], val)
        else:
            node.register_parameter(parts[-1], nn.Parameter(val, requires_grad=requires_grad))


class _Hosted(_TreeWatch):
    """A module whose forward runs on an lns engine.  The engine belongs to the
    outermost constructed object (`_owner`); nested views share it."""

    def _init_host(self, cfg=None, owner=None, prefix=""):
        object.__setattr__(self, "_owner_ref", owner if owner is not None else self)
        object.__setattr__(self, "_prefix", prefix)
        if owner is None:
            object.__setattr__(self, "_eng", _engine.Engine(cfg))
            object.__setattr__(self, "_sig", None)
            object.__setattr__(self, "_flat", None)
            object.__setattr__(self, "_flat_epoch", -1)

    @property
    def _owner(self):
        return self._owner_ref

    def _weights_signature(self):
        """(flat [(key, tensor)] list of the owner's CURRENT parameter tree, hashable signature of its contents)."""
        own = self._owner
        flat = own._flat
        if flat is None or own._flat_epoch != _TREE_EPOCH[0]:
            flat = [(k, t) for k, t in list(own.named_parameters()) + list(own.named_buffers())]
            object.__setattr__(own, "_flat", flat)
            object.__setattr__(own, "_flat_epoch", _TREE_EPOCH[0])
        return flat, tuple((id(t), t.data_ptr(), t._version) for _, t in flat)

    def _engine(self, like):
        """Engine with the current weights resident on `like`'s device."""
        own = self._owner
        if not isinstance(like, torch.Tensor) or not like.is_cuda:
            raise LnsError("the LNS drop-in runs on HIP device tensors only (input is on %s); there is "
                           "no CPU fallback -- use the reference implementation on CPU"
                           % (getattr(like, "device", "host")))
        # The tensors of the parameter tree are looked up once per TREE EPOCH (the walk costs 0.5 ms; anything that can
        # replace a Parameter / buffer object bumps _TREE_EPOCH, see _TreeWatch); a call compares (object identity,
        # storage pointer, version) of each tensor and re-packs the weights when something changed.
        flat, wsig = own._weights_signature()
        dev = like.device.index if like.device.index is not None else torch.cuda.current_device()
        sig = (dev, wsig)
        if own._sig != sig:
            own._eng.load_weights({k: t.detach().to("cpu", torch.float32).numpy() for k, t in flat}, dev)
            object.__setattr__(own, "_sig", sig)
        return own._eng


# ---------------------------------------------------------------------------
class SimpleAutoencoder(_Hosted):
    """modules/autoencoder2d{,_nonsquared,_half_periodic}.py `SimpleAutoencoder`."""
    _ae_kind = LNS_AE_SQUARE

    def __init__(self, args, _owner=None, _prefix=""):
        super().__init__()
        self.args = args
        if _owner is None:
            cfg = _engine.make_config(args, ae_kind=self._ae_kind, prop_kind=LNS_PROP_NONE)
            self._init_host(cfg=cfg)
            _grow_tree(self, self._eng.params, requires_grad=False)      # no backward through the autoencoder (module docstring)
        else:
            self._init_host(owner=_owner, prefix=_prefix)
            _grow_tree(self, [p for p in _owner._eng.params if p[0].startswith(_prefix)], strip=_prefix, requires_grad=False)

    def encode(self, x):
        _no_backward("SimpleAutoencoder.encode", x, params=self.parameters())
        with torch.no_grad():
            return self._engine(x).encode(x)

    def decode(self, z):
        _no_backward("SimpleAutoencoder.decode", z, params=self.parameters())
        with torch.no_grad():
            return self._engine(z).decode(z)

    def forward(self, x):
        return self.decode(self.encode(x))

    def _validate(self, x, param, norm):
        """x [B,T,C,H,W] or [N,C,H,W] (scored as N trajectories of one step) -> (frame_wise, seq_wise)."""
        _no_backward("SimpleAutoencoder.validate", x, params=self.parameters())
        if x.dim() == 4:
            x = x[:, None]
        with torch.no_grad():
            res = self._engine(x).autoencode_eval(x, param=param, **norm)
        return res.frame, res.seq

    def validate(self, x, **norm):
        """The validation loop of the stage-1 scripts (train_stage1_ns2d.py:104-124; train_stage1_SW.py:107-110) in one call,
            x_hat = denormalize(autoencoder(x[:, t])); relative_lp_loss(x_hat, denormalize(x[:, t]), reduce_dim=(-1, -2))
        over every step of x [B,T,C,H,W] (or [N,C,H,W]: N single frames), without storing the reconstruction.  `norm` as in
        `metrics.relative_l2`.  Returns (frame_wise [B,T,C], seq_wise [B,C]): the bits of
        `metrics.relative_l2(autoencoder(x), x, **norm)`."""
        return self._validate(x, None, norm)

    def load_checkpoint(self, path, device=None):
        ckpt = torch.load(path, map_location=device)
        self.load_state_dict(ckpt, strict=True)


class SimpleAutoencoderNonSquared(SimpleAutoencoder):
    _ae_kind = LNS_AE_NONSQUARED


class SimpleAutoencoderHalfPeriodic(SimpleAutoencoder):
    _ae_kind = LNS_AE_HALF_PERIODIC


class ConditionalSimpleAutoencoder(SimpleAutoencoder):
    """modules/autoencoder2d_nonsquared.py:279-305: `CondEncoder` (:71-145, `CondResidualBlock`s conditioned on
    embed(fourier_embedding(param)), modules/cond_utils.py:58-128) + the plain non-squared Decoder.
    encode(x, param) / decode(z) / forward(x, param); state_dict keys as the reference's
    (`encoder.to_in.*`, `encoder.embed.*`, `encoder.layers.i.0.j.{conv1,conv2,shortcut,norm1,norm2,cond_emb}.*`,
    `encoder.layers.i.1.conv_layer.*`, `encoder.to_out_conv.*`, `encoder.to_out.*`, `decoder.model.*`, ...)."""
    _ae_kind = LNS_AE_NONSQUARED

    def __init__(self, args):
        if not getattr(args, "cond_encoder", False):
            args = types.SimpleNamespace(**vars(args))
            args.cond_encoder = True
        super().__init__(args)

    def encode(self, x, param):
        _no_backward("ConditionalSimpleAutoencoder.encode", x, params=self.parameters())
        with torch.no_grad():
            return self._engine(x).encode(x, param)

    def forward(self, x, param):
        return self.decode(self.encode(x, param))

    def validate(self, x, param, **norm):
        """SimpleAutoencoder.validate for the conditional encoder (train_stage1_twophase.py:111-114): param holds one value
        per trajectory of x [B,T,C,H,W] (per frame of [N,C,H,W])."""
        return self._validate(x, param, norm)

    def load_checkpoint(self, path):
        self.load_state_dict(torch.load(path), strict=True)


# ---------------------------------------------------------------------------
class SimpleCNN(_Hosted):
    """Latent propagator `SimpleCNN` of the stage-2 scripts.  `pad` = (mode_y, mode_x)."""
    _prop_kind = LNS_PROP_PLAIN
    _pad = (LNS_PAD_CIRCULAR, LNS_PAD_CIRCULAR)

    def __init__(self, latent_dim, prop_n_block, prop_n_embd, dilation=2, _owner=None, _prefix="",
                 _cond_emb_dim=None):
        super().__init__()
        self.latent_dim = latent_dim
        self.prop_n_block = prop_n_block
        self.prop_n_embd = prop_n_embd
        if _owner is None:
            a = types.SimpleNamespace(latent_dim=latent_dim, prop_n_block=prop_n_block, prop_n_embd=prop_n_embd,
                                      dilation=dilation, cond_emb_dim=_cond_emb_dim or latent_dim)
            cfg = _engine.make_config(a, ae_kind=LNS_AE_NONE, prop_kind=self._prop_kind, prop_pad=self._pad)
            self._init_host(cfg=cfg)
            _grow_tree(self, self._eng.params)
        else:
            self._init_host(owner=_owner, prefix=_prefix)
            _grow_tree(self, [p for p in _owner._eng.params if p[0].startswith(_prefix)], strip=_prefix)

    def forward(self, z, param=None):
        _no_backward("SimpleCNN.forward", z, params=self.parameters())
        with torch.no_grad():
            return self._engine(z).propagate(z, param)


class SimpleCNNHalfPeriodic(SimpleCNN):       # train_stage2_SW.py:56-87 (periodic_direction='x')
    _pad = (LNS_PAD_ZEROS, LNS_PAD_CIRCULAR)


class SimpleCNNZeros(SimpleCNN):              # train_stage2_twophase.py:56-87 (padding_mode='zeros')
    _pad = (LNS_PAD_ZEROS, LNS_PAD_ZEROS)


class SimpleCNNConditional(SimpleCNN):        # train_stage2_twophase_conditional.py:78-121
    _prop_kind = LNS_PROP_CONDITIONAL
    _pad = (LNS_PAD_ZEROS, LNS_PAD_ZEROS)

    def __init__(self, latent_dim, cond_emb_dim, prop_n_block, prop_n_embd, dilation=2, _owner=None, _prefix=""):
        super().__init__(latent_dim, prop_n_block, prop_n_embd, dilation, _owner=_owner, _prefix=_prefix,
                         _cond_emb_dim=cond_emb_dim)
        self.cond_emb_dim = cond_emb_dim

    def forward(self, z, param):
        _no_backward("SimpleCNN.forward", z, params=self.parameters())
        with torch.no_grad():
            return self._engine(z).propagate(z, param)


# ---------------------------------------------------------------------------
class _LatentRolloutFn(torch.autograd.Function):
    """z_pred = rollout(z0; propagator parameters) on the HIP engine, differentiable w.r.t. the parameters, z0 and -- the
    conditional model -- `param` (include/lns.h "training rollout", lns_train_backward_ex; csrc/lns_train.inc).  The
    parameters are read from their device tensors at every call, so an optimiser's in-place updates need no re-upload."""

    @staticmethod
    def forward(ctx, own, names, T, z0, param, *tensors):
        if not z0.is_cuda:
            raise LnsError("the LNS drop-in runs on HIP device tensors only (input is on %s); there is no CPU fallback" % z0.device)
        eng = own._eng
        params = {k: t.detach() for k, t in zip(names, tensors)}
        for k, t in params.items():
            if not t.is_cuda:
                raise LnsError("training rollout: parameter %s is not on the HIP device (call model.cuda())" % k)
        with torch.cuda.device(z0.device):
            z_pred, ws = eng.train_forward(params, z0.detach(), T, param=param)
        ctx.own, ctx.names, ctx.ws = own, names, ws
        if isinstance(param, torch.Tensor):
            ctx.param_shape, ctx.param_dtype = param.shape, param.dtype
        ctx.save_for_backward(z0, z_pred, *tensors)
        return z_pred

    @staticmethod
    def backward(ctx, grad_out):
        z0, z_pred, *tensors = ctx.saved_tensors
        params = {k: t.detach() for k, t in zip(ctx.names, tensors)}
        gp = None
        with torch.cuda.device(z0.device):
            if ctx.needs_input_grad[4]:
                grads, gz, gp = ctx.own._eng.train_backward(params, z0, z_pred, grad_out.contiguous().float(), ctx.ws,
                                                            need_z_grad=ctx.needs_input_grad[3], need_param_grad=True)
                gp = gp.reshape(ctx.param_shape).to(ctx.param_dtype)
            else:
                grads, gz = ctx.own._eng.train_backward(params, z0, z_pred, grad_out.contiguous().float(), ctx.ws,
                                                        need_z_grad=ctx.needs_input_grad[3])
        out = [None, None, None, gz, gp]
        for i, k in enumerate(ctx.names):
            out.append(grads[k] if ctx.needs_input_grad[5 + i] else None)
        return tuple(out)


# ---------------------------------------------------------------------------
class LatentDynamics(_Hosted):
    """`LatentDynamics` of train_stage2_ns2d.py:90-158 (and the SW / two-phase variants)."""
    _family = "ns2d"
    _ae_cls = SimpleAutoencoder
    _prop_cls = SimpleCNN
    _ae_attr = "vq_ae"
    _conditional = False

    def __init__(self, args):
        super().__init__()
        if getattr(args, "family", None) is None:
            args = types.SimpleNamespace(**vars(args))
            args.family = self._family
        self.args = args
        self.latent_resolution = args.latent_resolution
        self.latent_dim = args.latent_dim
        cfg = _engine.make_config(args, ae_kind=self._ae_cls._ae_kind, prop_kind=self._prop_cls._prop_kind,
                                  ae_prefix=self._ae_attr + ".", prop_prefix="propagator.",
                                  prop_pad=self._prop_cls._pad)
        self._init_host(cfg=cfg)
        ae = self._ae_cls(args, _owner=self, _prefix=self._ae_attr + ".")
        self.add_module(self._ae_attr, ae)
        if self._conditional:
            prop = self._prop_cls(args.latent_dim, args.latent_dim, args.prop_n_block, args.prop_n_embd,
                                  args.dilation, _owner=self, _prefix="propagator.")
        else:
            prop = self._prop_cls(args.latent_dim, args.prop_n_block, args.prop_n_embd, args.dilation,
                                  _owner=self, _prefix="propagator.")
        self.propagator = prop

    @property
    def _ae(self):
        return getattr(self, self._ae_attr)

    def load_autoencoder(self, args):
        print("Loading pretrained autoencoder from {}".format(args.pretrained_checkpoint_path))
        self._ae.load_checkpoint(args.pretrained_checkpoint_path, device=getattr(args, "device", None))
        print("Pretrained autoencoder loaded successfully")
        for p in self._ae.parameters():
            p.requires_grad = False
        self._ae.eval()

    @torch.no_grad()
    def x_to_z(self, x):
        return self._ae.encode(x)

    @torch.no_grad()
    def z_to_x(self, z):
        return self._ae.decode(z)

    def forward(self, z_in, z_out, *rest):
        """forward(z_in, z_out, loss_fn) -- conditional: forward(z_in, z_out, param, loss_fn): the loss of the latent
        rollout started at z_in[:, 0] against the pre-encoded targets z_out [B,t_out,c,h,w]
        (train_stage2_ns2d.py:126-141; conditional train_stage2_twophase_conditional.py:160-175).
        With autograd enabled (training, train_stage2_ns2d.py:213-215) the rollout runs through `_LatentRolloutFn`:
        the HIP training forward keeps a tape and `loss.backward()` runs the HIP backward through time, filling `.grad`
        of the propagator's parameters -- and of `param` when it requires grad (model(z_in, z_out,
        param.requires_grad_(), loss_fn) fills param.grad; otherwise no gradient w.r.t. it is computed).  Under
        torch.no_grad() (validation) it is the inference rollout."""
        if torch.is_grad_enabled():
            if len(rest) != (2 if self._conditional else 1):
                raise TypeError("forward() takes (z_in, z_out, param, loss_fn)" if self._conditional else "forward() takes (z_in, z_out, loss_fn)")
            cparam, loss_fn = (rest[0], rest[1]) if self._conditional else (None, rest[0])
            if z_in.dim() != 5 or z_in.shape[1] != 1:
                raise AssertionError("z_in must be [B,1,c,h,w] (t_in == 1)")
            z0 = z_in[:, 0].contiguous().float()
            own = self._owner
            named = dict(own.named_parameters())
            names = [k for k in named if k.startswith("propagator.")]
            z_pred = _LatentRolloutFn.apply(own, names, int(z_out.shape[1]), z0, cparam, *[named[k] for k in names])
            return loss_fn(z_pred, z_out)
        param = None
        if self._conditional:
            if len(rest) != 2:
                raise TypeError("forward() takes (z_in, z_out, param, loss_fn)")
            param, loss_fn = rest
        else:
            if len(rest) != 1:
                raise TypeError("forward() takes (z_in, z_out, loss_fn)")
            loss_fn, = rest
        if z_in.dim() != 5 or z_in.shape[1] != 1:
            raise AssertionError("z_in must be [B,1,c,h,w] (t_in == 1)")
        z0 = z_in[:, 0].contiguous()
        z_pred, _ = self._engine(z0).rollout_latent(z0, z_out.shape[1], param=param, to_x=False)
        return loss_fn(z_pred, z_out)

    def assimilate(self, x0, y_obs, obs_steps, *rest, iters=40, weights=None, chunk=32, method="adam", outer=3, cg_iters=8,
                   damping=0.0, **fit):
        """assimilate(x0, y_obs, obs_steps, iters=...) -- conditional: assimilate(x0, y_obs, obs_steps, param, iters=...):
        which initial latent makes the rollout agree with ALL the observed frames, and (conditional model) which `param`
        explains them.  x0 [B,C,Ly,Lx]: the frame the forecast would start from -- its encoding is the start of the fit and
        its background; y_obs [B,n_obs,C,Ly,Lx]: the frames observed at the 0-based rollout steps `obs_steps` (step 0 = one
        propagator step after x0), encoded `chunk` frames per call as metrics.encode_dataset does.  `fit`: LatentFit's
        arguments (lr_state, lr_param, betas, eps, background, fit_state, fit_param).  Returns fit.FitResult (z0, param,
        loss [iters, B], per [B, n_obs]); `model._engine(z0).rollout_latent(z0, steps, param=...)` forecasts from it.
        With a conditional ENCODER fitting `param` is refused: the encoding of the observations would depend on the
        unknown (LatentFit.run on latents has no such limit).
        method="gauss_newton": the state is fitted by LatentFit.run_gauss_newton -- `outer` iterations of `cg_iters`
        conjugate-gradient steps on the Gauss-Newton operator, Levenberg `damping` -- instead of `iters` Adam steps; loss is
        then [outer + 1, B].  `param` is a known input there: fit_param=True is refused (the tangent-linear rollout has no
        param direction)."""
        from . import fit as _fit
        from . import metrics as _metrics
        if method not in ("adam", "gauss_newton"):
            raise LnsError("assimilate: method must be 'adam' or 'gauss_newton', got %r" % (method,))
        if method == "gauss_newton" and fit.get("fit_param"):
            raise LnsError("assimilate: method='gauss_newton' fits the state only: the tangent-linear rollout has no param "
                           "direction, so there is no Gauss-Newton product for param; drop fit_param=True (param is then a "
                           "known input), or use method='adam'")
        param = None
        if self._conditional:
            if not rest:
                raise TypeError("assimilate() missing required argument: 'param'")
            param, rest = rest[0], rest[1:]
        if rest:
            raise TypeError("assimilate() takes (x0, y_obs, obs_steps, param, ...)" if self._conditional
                            else "assimilate() takes (x0, y_obs, obs_steps, ...)")
        fitter = _fit.LatentFit(self, **fit)
        cond_enc = bool(getattr(self.args, "cond_encoder", False))
        if cond_enc and fitter.fit_param and method == "adam":
            raise LnsError("assimilate: the encoder is conditional, so the encoding of the observations would depend on the "
                           "param being fitted; pass fit_param=False, or fit latents with lns_amd.fit.LatentFit.run")
        x0 = self._fields(x0)
        if y_obs.dim() != 5 or y_obs.shape[0] != x0.shape[0] or y_obs.shape[2:] != x0.shape[1:]:
            raise LnsError("y_obs must be [B,n_obs,C,Ly,Lx] matching x0 %s, got %s" % (tuple(x0.shape), tuple(y_obs.shape)))
        B, n_obs = int(y_obs.shape[0]), int(y_obs.shape[1])
        with torch.no_grad():
            enc_p = param if cond_enc else None
            z0 = _metrics.encode_dataset(self._ae, x0, chunk=chunk, out_device=x0.device, param=enc_p)
            frames = y_obs.reshape((B * n_obs,) + tuple(y_obs.shape[2:]))
            enc_po = torch.as_tensor(param).reshape(B, 1).expand(B, n_obs).reshape(-1) if cond_enc else None
            z_obs = _metrics.encode_dataset(self._ae, frames, chunk=chunk, out_device=x0.device, param=enc_po)
        z_obs = z_obs.reshape((B, n_obs) + tuple(z_obs.shape[1:]))
        if method == "gauss_newton":
            return fitter.run_gauss_newton(z0, z_obs, obs_steps, param=param, weights=weights, outer=outer, cg_iters=cg_iters,
                                           damping=damping)
        return fitter.run(z0, z_obs, obs_steps, param=param, weights=weights, iters=iters)

    @torch.no_grad()
    def assimilate_ensemble(self, x0, y_obs, obs_steps, *rest, rinv, inflation=1.0, window=1, generator=None, param_spread=0.0,
                            loc_radius=None, loc_boundary="auto", **norm):
        """assimilate_ensemble(x0, y_obs, obs_steps, members, noise_level, rinv=...) -- conditional:
        assimilate_ensemble(x0, y_obs, obs_steps, param, members, noise_level, rinv=...): an ensemble of forecasts from x0
        corrected by SPARSE observations of the decoded fields (a few sensors, one channel, a masked region) with an ensemble
        transform Kalman filter (lns_amd.enkf.EnsembleFilter) -- where `assimilate` needs complete frames it can encode.
        x0 [B,C,Ly,Lx] is encoded and perturbed as `predict_ensemble` does without a control member; y_obs
        [B,n_obs,C,Ly,Lx]: the normalised observations at the rollout steps `obs_steps` (`assimilate`'s convention: step 0 =
        one propagator step after x0), any value where rinv is 0; rinv: the inverse observation-error variance per value,
        [C,Ly,Lx], [n_obs,C,Ly,Lx] or [B,n_obs,C,Ly,Lx], in the units `norm` gives (`validate`'s arguments; none:
        normalised units); inflation >= 1; window: observations taken in per analysis; param_spread > 0: param [B] becomes
        param + randn * param_spread per member and is estimated with the state (also with a conditional encoder).
        loc_radius (None: the global filter): the Gaspari-Cohn half-width, in latent pixels, of the localised filter
        (lns_amd.enkf.LocalEnsembleFilter: one transform per latent pixel; returns enkf.LocalEnKFResult), loc_boundary its
        boundary rule ("auto": the model's padding per axis).
        Returns enkf.EnKFResult; `model._engine(z).rollout_latent_ensemble(result.z, steps, param=result.param)` forecasts
        from the analysis, which stands at the last observed step."""
        from . import enkf as _enkf
        param = None
        if self._conditional:
            if not rest:
                raise TypeError("assimilate_ensemble() missing required argument: 'param'")
            param, rest = rest[0], rest[1:]
        if len(rest) != 2:
            raise TypeError("assimilate_ensemble() takes (x0, y_obs, obs_steps, param, members, noise_level)" if self._conditional
                            else "assimilate_ensemble() takes (x0, y_obs, obs_steps, members, noise_level)")
        members, noise_level = int(rest[0]), float(rest[1])
        if members < 2:
            raise LnsError("the filter needs at least 2 members, got %d" % members)
        x0 = self._fields(x0)
        if y_obs.dim() != 5 or y_obs.shape[0] != x0.shape[0] or y_obs.shape[2:] != x0.shape[1:]:
            raise LnsError("y_obs must be [B,n_obs,C,Ly,Lx] matching x0 %s, got %s" % (tuple(x0.shape), tuple(y_obs.shape)))
        if bool(getattr(self.args, "cond_encoder", False)):
            from . import metrics as _metrics        # (the encoder reads the first-guess param; the filter then moves the members')
            z0 = _metrics.encode_dataset(self._ae, x0, chunk=32, out_device=x0.device, param=param)
            B = z0.shape[0]
            z = z0[:, None] + torch.randn((B, members) + tuple(z0.shape[1:]), device=z0.device, dtype=z0.dtype,
                                          generator=generator) * noise_level
        else:
            z = self._ensemble_latents(x0, members, noise_level, generator, False)
        if param is not None and float(param_spread) > 0.0:
            p = torch.as_tensor(param, device=z.device, dtype=torch.float32).reshape(-1, 1)
            param = p + torch.randn((p.shape[0], members), device=z.device, generator=generator) * float(param_spread)
        flt = _enkf.EnsembleFilter(self, inflation) if loc_radius is None else \
            _enkf.LocalEnsembleFilter(self, loc_radius, inflation, loc_boundary)
        return flt.run(z.contiguous(), y_obs, rinv, obs_steps, window=window, param=param, **norm)

    def lyapunov(self, x, steps, *rest, k=4, **kw):
        """lyapunov(x, steps, k=4, ...) -- conditional: lyapunov(x, steps, param, k=4, ...): the k leading finite-time
        Lyapunov exponents of the learned dynamics along the `steps`-step forecast started at the frame x [B,C,Ly,Lx]
        (its encoding is the start).  `kw`: TangentRollout.lyapunov's arguments (renorm, burn_in, chunk, generator, dt).
        Returns tangent.LyapunovResult (exponents [B,k], history, vectors [B,k,c,h,w], z_last); 1 / exponents[:, 0] is
        the e-folding time of a perturbation in units of dt, and `vectors` are the growing directions at z_last."""
        from . import metrics as _metrics
        from . import tangent as _tangent
        param = None
        if self._conditional:
            if not rest:
                raise TypeError("lyapunov() missing required argument: 'param'")
            param, rest = rest[0], rest[1:]
        if rest:
            raise TypeError("lyapunov() takes (x, steps, param, k=...)" if self._conditional else "lyapunov() takes (x, steps, k=...)")
        roll = _tangent.TangentRollout(self)
        x = self._fields(x)
        with torch.no_grad():
            enc_p = param if bool(getattr(self.args, "cond_encoder", False)) else None
            z0 = _metrics.encode_dataset(self._ae, x, chunk=32, out_device=x.device, param=enc_p)
        return roll.lyapunov(z0, steps, k=k, param=param, **kw)

    @staticmethod
    def _fields(x):
        # SW / two-phase loaders hand [B,1,C,H,W]; the reference squeezes (B=1 safe here)
        if x.dim() == 5 and x.shape[1] == 1:
            x = x[:, 0]
        return x

    @torch.no_grad()
    def predict(self, x, steps, *rest, to_x=False, return_latents=False, keep_steps=None):
        """predict(x, steps, to_x=False) -- conditional: predict(x, steps, param, to_x=False).
        keep_steps (with to_x=True; ints, a range, or a slice such as slice(None, None, 5) for the `::5` the reference
        plots): only these steps are decoded -> [B, n_keep, C, Ly, Lx], the bits of predict(...)[:, keep_steps]."""
        param = None
        if self._conditional:
            if not rest:
                raise TypeError("predict() missing required argument: 'param'")
            param, rest = rest[0], rest[1:]
        if rest:
            to_x = rest[0]
        x = self._fields(x)
        return self._engine(x).rollout(x, steps, param=param, to_x=to_x, return_latents=return_latents, keep_steps=keep_steps)

    def _ensemble_latents(self, x, members, noise_level, generator, control):
        """x -> z [B, members, c, h, w]: z0 + randn * noise_level per member, member 0 left as z0 under control."""
        z0 = self.x_to_z(self._fields(x))
        B, c, h, w = z0.shape
        eps = torch.randn((B, members, c, h, w), device=z0.device, dtype=z0.dtype, generator=generator) * noise_level
        z = z0[:, None] + eps
        if control:
            z[:, 0] = z0
        return z

    @torch.no_grad()
    def predict_ensemble(self, x, steps, *rest, generator=None, control=True, keep_steps=None, return_var=True):
        """predict_ensemble(x, steps, members, noise_level) -- conditional: predict_ensemble(x, steps, param, members,
        noise_level): an ensemble forecast from the robustness the stage-2 training buys with its latent noise
        (z_in + randn_like(z_in) * noise_level, train_stage2_ns2d.py:211-212).  Encodes x once, perturbs the latent
        `members` times -- z[b, m] = z0[b] + randn * noise_level, member 0 left as z0 under control=True -- rolls every
        member out and returns the per-step mean, or (mean, var) with the unbiased variance over the members, of the
        decoded fields [B, n_keep, C, Ly, Lx]; the members' own fields are never stored.  generator: a torch.Generator on
        x's device for the noise.  param: [B] (shared by a trajectory's members) or [B, members].  keep_steps as for predict."""
        param = None
        if self._conditional:
            if not rest:
                raise TypeError("predict_ensemble() missing required argument: 'param'")
            param, rest = rest[0], rest[1:]
        if len(rest) != 2:
            raise TypeError("predict_ensemble() takes (x, steps, param, members, noise_level)" if self._conditional
                            else "predict_ensemble() takes (x, steps, members, noise_level)")
        members, noise_level = int(rest[0]), float(rest[1])
        if members < 1:
            raise LnsError("members must be at least 1, got %d" % members)
        z = self._ensemble_latents(x, members, noise_level, generator, control)
        return self._engine(z).rollout_latent_ensemble(z, steps, param=param, keep_steps=keep_steps, return_var=return_var)

    @torch.no_grad()
    def predict_quantiles(self, x, steps, *rest, quantiles=(0.05, 0.5, 0.95), thresholds=(), generator=None, control=True,
                          keep_steps=None, return_mean=False, return_var=False, **norm):
        """predict_quantiles(x, steps, members, noise_level) -- conditional: predict_quantiles(x, steps, param, members,
        noise_level): the ensemble forecast of `predict_ensemble` (same encode, same noise from the same generator state, same
        `control`) summarised per kept step and pixel by quantiles of the member values (a median, a band, the envelope)
        and by the share of the members above each threshold -- what a clamped or wall-zeroed channel needs where a mean and
        a variance say little.  Returns engine.EnsembleQuantiles; return_mean / return_var add predict_ensemble's mean and
        variance (same bits).  thresholds: scalars or per-channel sequences, in the units of the values; `norm` as in
        `validate` (none: normalised values); keep_steps as for predict."""
        param = None
        if self._conditional:
            if not rest:
                raise TypeError("predict_quantiles() missing required argument: 'param'")
            param, rest = rest[0], rest[1:]
        if len(rest) != 2:
            raise TypeError("predict_quantiles() takes (x, steps, param, members, noise_level)" if self._conditional
                            else "predict_quantiles() takes (x, steps, members, noise_level)")
        members, noise_level = int(rest[0]), float(rest[1])
        if members < 1:
            raise LnsError("members must be at least 1, got %d" % members)
        z = self._ensemble_latents(x, members, noise_level, generator, control)
        return self._engine(z).rollout_latent_ensemble_quantiles(z, steps, quantiles=quantiles, thresholds=thresholds, param=param,
                                                                 keep_steps=keep_steps, return_mean=return_mean,
                                                                 return_var=return_var, **norm)

    @torch.no_grad()
    def validate_ensemble(self, x, y, *rest, generator=None, control=True, keep_steps=None, **norm):
        """validate_ensemble(x, y, members, noise_level, **norm) -- conditional: validate_ensemble(x, y, param, members,
        noise_level, **norm): the ensemble forecast of `predict_ensemble` over T = y.shape[1] steps (same encode, same noise
        from the same generator state, same `control`), scored against the normalised truth y [B,T,C,Ly,Lx] as it is
        decoded: relative L2 and RMSE of the ensemble mean, spread, fair CRPS and the rank histogram per kept step and
        channel (engine.EnsembleScores; `metrics.spread_skill_ratio`).  Neither the members' fields nor their mean are
        stored.  `norm` as in `validate`; keep_steps as for predict (None: every step)."""
        param = None
        if self._conditional:
            if not rest:
                raise TypeError("validate_ensemble() missing required argument: 'param'")
            param, rest = rest[0], rest[1:]
        if len(rest) != 2:
            raise TypeError("validate_ensemble() takes (x, y, param, members, noise_level)" if self._conditional
                            else "validate_ensemble() takes (x, y, members, noise_level)")
        members, noise_level = int(rest[0]), float(rest[1])
        if members < 2:
            raise LnsError("scoring an ensemble needs at least 2 members, got %d" % members)
        z = self._ensemble_latents(x, members, noise_level, generator, control)
        return self._engine(z).rollout_latent_ensemble_eval(z, y, param=param, keep_steps=keep_steps, **norm)

    @torch.no_grad()
    def validate_exceedance(self, x, y, *rest, thresholds, generator=None, control=True, keep_steps=None, **norm):
        """validate_exceedance(x, y, members, noise_level, thresholds=...) -- conditional: validate_exceedance(x, y, param,
        members, noise_level, thresholds=...): the ensemble forecast of `validate_ensemble` over T = y.shape[1] steps (same
        encode, same noise from the same generator state, same `control`) verified as an event forecast: for every kept step,
        threshold and channel the integer table of how many pixels had n of the members above the threshold while the truth
        was / was not above it, counted as the members are decoded (engine.EnsembleExceedance).  `metrics.brier_scores`,
        `reliability_curve`, `roc_curve` and `contingency_scores` turn a table into scores; `predict_quantiles`' `prob` is the
        forecast they verify.  thresholds: scalars or per-channel sequences, in the units of the values; `norm` as in
        `validate` (none: normalised values); keep_steps as for predict (None: every step).  members >= 1."""
        param = None
        if self._conditional:
            if not rest:
                raise TypeError("validate_exceedance() missing required argument: 'param'")
            param, rest = rest[0], rest[1:]
        if len(rest) != 2:
            raise TypeError("validate_exceedance() takes (x, y, param, members, noise_level)" if self._conditional
                            else "validate_exceedance() takes (x, y, members, noise_level)")
        members, noise_level = int(rest[0]), float(rest[1])
        if members < 1:
            raise LnsError("members must be at least 1, got %d" % members)
        z = self._ensemble_latents(x, members, noise_level, generator, control)
        return self._engine(z).rollout_latent_ensemble_exceed(z, y, None, thresholds, param=param, keep_steps=keep_steps, **norm)

    @torch.no_grad()
    def validate(self, x, y, *rest, keep_steps=(), **norm):
        """validate(x, y, **norm) -- conditional: validate(x, y, param, **norm): the body of the reference's validation
        loop (train_stage2_ns2d.py:249-263) in one call,
            y_hat = denormalize(predict(x, T, to_x=True)); y = denormalize(y)
            frame_wise = relative_lp_loss(y_hat, y, reduce_dim=(3, 4)); seq_wise = relative_lp_loss(y_hat, y, reduce_dim=(1, 3, 4))
        with T = y.shape[1] and the decoded rollout scored group by group as it is decoded: y_hat [B,T,C,Ly,Lx] is never
        stored.  `norm` restates the dataset's denormalize as in `metrics.relative_l2` (mean, std, eps,
        zero_wall_channels, clamp_channels, clamp; e.g. `**metrics.twophase_spec(...)`).  Returns (frame_wise [B,T,C],
        seq_wise [B,C], decoded frames [B,len(keep_steps),C,Ly,Lx] or None -- the few the reference plots)."""
        param = None
        if self._conditional:
            if not rest:
                raise TypeError("validate() missing required argument: 'param'")
            param, rest = rest[0], rest[1:]
        if rest:
            raise TypeError("validate() takes (x, y, param, **norm)" if self._conditional else "validate() takes (x, y, **norm)")
        x = self._fields(x)
        return self._engine(x).rollout_eval(x, y, param=param, keep_steps=keep_steps, **norm)

    @torch.no_grad()
    def validate_spectrum(self, x, y, *rest, spectrum_steps=None, keep_steps=(), spectrum_basis="dft", **norm):
        """validate_spectrum(x, y, **norm) -- conditional: validate_spectrum(x, y, param, **norm): `validate` with the
        shell-summed energy spectra of forecast, truth and error of the steps `spectrum_steps` (a sequence, range or slice;
        None: every step), taken as the steps are decoded.  Returns engine.EvalSpectra: frame, seq, frames as `validate`
        returns them, spectra [B,n,C,3,S] (S = metrics.spectrum_bins(Ly, Lx); rows forecast, truth, error) and the steps.
        Bins are index wavenumbers; under spectrum_basis="dft" a spectrum of a non-periodic family carries the leakage of the
        walls: spectrum_basis="auto" (or "dct" / a pair (y, x)) takes a DCT-II on the axes with walls, S =
        metrics.spectrum_bins(Ly, Lx, basis) bins at metrics.spectrum_wavenumbers."""
        param = None
        if self._conditional:
            if not rest:
                raise TypeError("validate_spectrum() missing required argument: 'param'")
            param, rest = rest[0], rest[1:]
        if rest:
            raise TypeError("validate_spectrum() takes (x, y, param, **norm)" if self._conditional
                            else "validate_spectrum() takes (x, y, **norm)")
        x = self._fields(x)
        return self._engine(x).rollout_eval_spectrum(x, y, param=param, keep_steps=keep_steps, spectrum_steps=spectrum_steps,
                                                     basis=spectrum_basis, **norm)

    @torch.no_grad()
    def validate_stats(self, x, y, *rest, stats_steps=None, hist=None, spectrum_steps=(), keep_steps=(), spectrum_basis="dft",
                       **norm):
        """validate_stats(x, y, **norm) -- conditional: validate_stats(x, y, param, **norm): `validate` with the per-plane
        field statistics (metrics.FIELD_STATS: means, variances, correlation, gradient-domain error, extrema) of the steps
        `stats_steps` (a sequence, range or slice; None: every step) and, with hist = (nbins, lo, hi), the value histograms
        of forecast and truth, taken as the steps are decoded; `spectrum_steps` adds validate_spectrum's spectra in the
        same pass.  Returns engine.EvalStats.  metrics.correlation_time turns the corr column into a decorrelation step."""
        param = None
        if self._conditional:
            if not rest:
                raise TypeError("validate_stats() missing required argument: 'param'")
            param, rest = rest[0], rest[1:]
        if rest:
            raise TypeError("validate_stats() takes (x, y, param, **norm)" if self._conditional
                            else "validate_stats() takes (x, y, **norm)")
        x = self._fields(x)
        return self._engine(x).rollout_eval_stats(x, y, param=param, keep_steps=keep_steps, stats_steps=stats_steps, hist=hist,
                                                  spectrum_steps=spectrum_steps, spectrum_basis=spectrum_basis, **norm)

    @torch.no_grad()
    def validate_maps(self, x, y, *rest, map_steps=None, stats_steps=(), hist=None, spectrum_steps=(), keep_steps=(),
                      spectrum_basis="dft", **norm):
        """validate_maps(x, y, **norm) -- conditional: validate_maps(x, y, param, **norm): `validate` with the per-pixel time
        maps (metrics.TIME_MAPS: time-mean of forecast and truth, temporal variances and covariance, mean squared and largest
        error) over the steps `map_steps` (None: every step; slice(from, None, every) or (from, every) for burn-in and
        thinning), accumulated as the steps are decoded; `stats_steps` / `hist` and `spectrum_steps` add validate_stats'
        statistics and validate_spectrum's spectra in the same pass.  Returns engine.EvalMaps.  metrics.rmse_map and
        metrics.temporal_correlation derive the usual maps from it."""
        from .engine import normalize_map_steps
        normalize_map_steps(map_steps)                  # a ValueError before anything touches the device
        param = None
        if self._conditional:
            if not rest:
                raise TypeError("validate_maps() missing required argument: 'param'")
            param, rest = rest[0], rest[1:]
        if rest:
            raise TypeError("validate_maps() takes (x, y, param, **norm)" if self._conditional
                            else "validate_maps() takes (x, y, **norm)")
        x = self._fields(x)
        return self._engine(x).rollout_eval_maps(x, y, param=param, keep_steps=keep_steps, map_steps=map_steps,
                                                 stats_steps=stats_steps, hist=hist, spectrum_steps=spectrum_steps,
                                                 spectrum_basis=spectrum_basis, **norm)

    @torch.no_grad()
    def validate_flow(self, x, y, *rest, flow_steps=None, u=0, v=1, dx=1.0, dy=1.0, boundary="auto", vort_hist=None,
                      stats_steps=(), hist=None, spectrum_steps=(), keep_steps=(), spectrum_basis="dft", **norm):
        """validate_flow(x, y, **norm) -- conditional: validate_flow(x, y, param, **norm): `validate` with the flow diagnostics
        (metrics.FLOW_STATS: kinetic energy, enstrophy, rms divergence, vorticity error and cosine, velocity error, extrema) of
        the steps `flow_steps` (a sequence, range or slice; None: every step) across the velocity channels u (x-component)
        and v, taken as the steps are decoded: does the forecast stay divergence-free like the truth, does it keep the energy
        and the enstrophy, how wrong is its vorticity.  dx / dy: the grid spacings; boundary: "periodic", "wall", a pair
        (y, x) or "auto" (periodic where the autoencoder pads circularly); vort_hist = (nbins, lo, hi): the vorticity
        histograms of forecast and truth; keep_steps: the kept frames and their vorticity; `stats_steps` / `hist` and
        `spectrum_steps` add validate_stats' statistics and validate_spectrum's spectra in the same pass.  `norm` restates the
        dataset's denormalize, zero_wall_channels and clamp included.  Returns engine.EvalFlow."""
        param = None
        if self._conditional:
            if not rest:
                raise TypeError("validate_flow() missing required argument: 'param'")
            param, rest = rest[0], rest[1:]
        if rest:
            raise TypeError("validate_flow() takes (x, y, param, **norm)" if self._conditional
                            else "validate_flow() takes (x, y, **norm)")
        x = self._fields(x)
        return self._engine(x).rollout_eval_flow(x, y, param=param, keep_steps=keep_steps, flow_steps=flow_steps, u=u, v=v, dx=dx,
                                                 dy=dy, boundary=boundary, vort_hist=vort_hist, stats_steps=stats_steps,
                                                 hist=hist, spectrum_steps=spectrum_steps, spectrum_basis=spectrum_basis, **norm)

    @torch.no_grad()
    def validate_attribution(self, x, y, *rest, keep_steps=(), return_latents=False, **norm):
        """validate_attribution(x, y, **norm) -- conditional: validate_attribution(x, y, param, **norm): `validate` with the
        error of every plane split into the autoencoder's floor and the propagator's drift -- which of the two separately
        trained parts to retrain.  Returns engine.EvalAttrib: frame, seq, frames as `validate` returns them; recon_* the
        relative L2 of the reconstruction D(E(y)) (what the stage-1 scripts validate); prop_* and cross_* with
        frame^2 = prop^2 + recon^2 + cross (metrics.attribution_shares); latent_* the relative drift of the propagated latent
        from E(y_t); recon_frames the reconstructions of keep_steps; z_true (return_latents) the encoded truth."""
        param = None
        if self._conditional:
            if not rest:
                raise TypeError("validate_attribution() missing required argument: 'param'")
            param, rest = rest[0], rest[1:]
        if rest:
            raise TypeError("validate_attribution() takes (x, y, param, **norm)" if self._conditional
                            else "validate_attribution() takes (x, y, **norm)")
        x = self._fields(x)
        return self._engine(x).rollout_eval_attrib(x, y, param=param, keep_steps=keep_steps, return_latents=return_latents, **norm)


class LatentDynamicsSW(LatentDynamics):                # train_stage2_SW.py:90-159
    _family = "sw_half_periodic"
    _ae_cls = SimpleAutoencoderHalfPeriodic
    _prop_cls = SimpleCNNHalfPeriodic


class LatentDynamicsSWNonSquared(LatentDynamics):       # BASELINE config 3 (SW through autoencoder2d_nonsquared)
    _family = "sw_nonsquared"
    _ae_cls = SimpleAutoencoderNonSquared
    _prop_cls = SimpleCNNHalfPeriodic


class LatentDynamicsTwoPhase(LatentDynamics):           # train_stage2_twophase.py:90-159
    _family = "twophase"
    _ae_cls = SimpleAutoencoderNonSquared
    _prop_cls = SimpleCNNZeros


class LatentDynamicsTwoPhaseConditional(LatentDynamics):  # train_stage2_twophase_conditional.py:124-193
    _family = "twophase_cond"
    _ae_cls = SimpleAutoencoderNonSquared
    _prop_cls = SimpleCNNConditional
    _ae_attr = "ae"
    _conditional = True


FAMILY_CLASSES = {
    "ns2d": LatentDynamics,
    "sw_half_periodic": LatentDynamicsSW,
    "sw_nonsquared": LatentDynamicsSWNonSquared,
    "twophase": LatentDynamicsTwoPhase,
    "twophase_cond": LatentDynamicsTwoPhaseConditional,
}


def build_dynamics(args):
    return FAMILY_CLASSES[args.family](args)

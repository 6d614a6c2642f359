"""`Stage2Trainer`: the inner loop of the stage-2 scripts as one device-resident call.

The reference's step (train_stage2_ns2d.py:210-216; same text in the SW / two-phase scripts)

    optim.zero_grad()
    loss = model(z_in, z_out[, param], F.smooth_l1_loss)
    loss.backward()
    optim.step()

becomes `loss = trainer.step(z_in, z_out[, param])`: training forward, smooth-L1 loss and its gradient, backward through
time and Adam are enqueued by ONE call of the C ABI (lns_train_step) -- no host synchronisation, no allocation.  What the
per-step Python of the autograd path does again and again is done once here: the propagator's parameter pointers are
resolved once (and again only when the drop-in's tree epoch moves or a tensor's storage changes -- the rule
`_Hosted._weights_signature` uses; a replaced Parameter object takes the old one's place in the optimiser), gradient buffers, Adam state and the workspace persist.

  * gradients: persistent buffers installed as each parameter's `.grad` (what `loss.backward()` would leave there);
  * Adam state: the optimiser's own (`lns_amd.optim.Adam`), so `CosineAnnealingLR`, `state_dict()` and resuming from a
    reference `optim_*.pt` go through the optimiser; lr / betas / eps / weight_decay are read from
    `optimizer.param_groups[0]` at every call;
  * the returned loss is a 0-dim view into a ring of `loss_ring` (default 4096) device floats: it keeps its value for that
    many further steps (read it, or `.clone()` it, before; a loop that reduces an epoch's losses at its end passes
    `loss_ring=len(train_loader)`).

Not in the reference's loop, but what a BPTT rollout at a higher learning rate asks for: `max_grad_norm` clips the global L2
norm of the propagator's gradients (torch.nn.utils.clip_grad_norm_'s formula) inside the same enqueue, an
`lns_amd.optim.AdamW` makes the weight decay decoupled, `skip_nonfinite` leaves parameters and Adam state alone when the
norm is inf / NaN.  Any of the three routes the step through lns_train_step_clip; without them the step is what it was.
  * `.grad` then holds the CLIPPED gradients, as after clip_grad_norm_; `trainer.grad_norm` is the norm before clipping of
    the last such step (a 0-dim view into a ring like the loss's), `trainer.skipped_steps` the device count of skipped steps;
  * the optimiser's `step` counts advance on a skipped step too (they live on the host, which does not look): the bias
    corrections move on, as they do under torch.amp's GradScaler only when it is told to -- documented, not hidden;
  * `step(update=False)` is the plain call: unclipped gradients, no norm.
"""
import ctypes

import torch

from . import dropin as _dropin
from . import engine as _engine
from . import optim as _optim
from ._lib import LnsError

LOSS_RING = 4096
WGRAD_FORMS = {"tile": 0, "split": 1}


def propagator_tensors(own, eng, who="Stage2Trainer"):
    """[(table index, key, Parameter)] of the propagator's tensors in the engine's parameter-table order, each checked to
    be what the device-resident calls read through a raw pointer: present in the model, on the HIP device, contiguous fp32
    of the table's shape.  The one rule by which Stage2Trainer and lns_amd.fit.LatentFit resolve parameter pointers."""
    prefix = eng.cfg.prop_prefix.decode()
    named = dict(own.named_parameters())
    out = []
    for i, (k, shape, isb) in enumerate(eng.params):
        if not k.startswith(prefix) or isb:
            continue
        p = named.get(k)
        if p is None:
            raise LnsError("%s: the model has no parameter %s" % (who, k))
        if not p.is_cuda:
            raise LnsError("%s: parameter %s is on %s; the training step runs on HIP device tensors only "
                           "(call model.cuda()); there is no CPU fallback" % (who, k, p.device))
        if p.dtype != torch.float32 or not p.is_contiguous() or tuple(p.shape) != tuple(shape):
            raise LnsError("%s: %s must be a contiguous fp32 tensor of shape %s" % (who, k, tuple(shape)))
        out.append((i, k, p))
    if not out:
        raise LnsError("%s: the model has no propagator parameters" % who)
    dev = out[0][2].device
    if any(p.device != dev for _, _, p in out):
        raise LnsError("%s: the propagator's parameters live on several devices" % who)
    return out


class Stage2Trainer:
    def __init__(self, model, optimizer=None, lr=1e-3, beta=1.0, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                 loss_ring=LOSS_RING, wgrad=None, max_grad_norm=None, skip_nonfinite=False):
        if not isinstance(model, _dropin.LatentDynamics):
            raise LnsError("Stage2Trainer needs a LatentDynamics drop-in (lns_amd.dropin), got %s" % type(model).__name__)
        if not beta > 0:
            raise LnsError("smooth-L1 beta must be > 0")
        self.model = model
        self.beta = float(beta)
        self._own = model._owner
        self._eng = self._own._eng
        if optimizer is None:
            optimizer = _optim.Adam(self._own.propagator.parameters(), lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        elif not isinstance(optimizer, _optim.Adam):
            raise LnsError("Stage2Trainer runs Adam on the device: pass an lns_amd.optim.Adam over the propagator's parameters "
                           "(a torch.optim.Adam state_dict loads into it), got %s" % type(optimizer).__name__)
        self.optimizer = optimizer
        if max_grad_norm is not None and not float(max_grad_norm) > 0:
            raise LnsError("max_grad_norm must be > 0 (None: no clipping), got %r" % (max_grad_norm,))
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self._norm = None              # ring of norms, parallel to the loss ring (clipped path only)
        self._norm_last = None
        self._key = None               # what the resolved pointers were taken from
        self._ws = {}                  # (device, B, T, h, w, bytes the engine asks for under its current options, clipped) -> workspace
        if wgrad is not None:          # None: the engine's option stays as it is
            self.set_wgrad(wgrad)
        self._loss = None
        self._loss_i = 0
        self._loss_ring = int(loss_ring)           # steps a returned loss keeps its value: size it to the logging interval
        if self._loss_ring < 1:
            raise LnsError("loss_ring must be >= 1")

    # -- one-time resolution -------------------------------------------------------------------------------------------
    def _resolve(self):
        eng, opt = self._eng, self.optimizer
        table = propagator_tensors(self._own, eng)
        group = opt.param_groups[0]
        in_group = {id(p) for p in group["params"]}
        n = len(eng.params)
        arrs = [(ctypes.c_void_p * n)() for _ in range(4)]
        params, grads, states = [], [], []
        old = {id(p): g for p, g in zip(getattr(self, "_params", ()), getattr(self, "_grads", ()))}
        prev = getattr(self, "_by_key", {})
        for i, k, p in table:
            if id(p) not in in_group and k in prev:
                # the Parameter object was replaced (`prop.in_proj.weight = nn.Parameter(...)`): the new tensor takes the
                # old one's place in the param group and, when the shape is the same, its Adam state
                q = prev[k]
                idx = [j for j, t in enumerate(group["params"]) if t is q]
                if idx:
                    group["params"][idx[0]] = p
                    in_group.add(id(p))
                    st_old = opt.state.pop(q, None)
                    if st_old and st_old["exp_avg"].shape == p.shape and st_old["exp_avg"].device == p.device:
                        opt.state[p] = st_old
            if id(p) not in in_group:
                raise LnsError("Stage2Trainer: parameter %s is not in optimizer.param_groups[0] (one group over "
                               "model.propagator.parameters() is what the step updates)" % k)
            g = old.get(id(p))
            if g is None or g.device != p.device:
                g = torch.zeros_like(p)
            st = opt.init_state(p)
            for name in ("exp_avg", "exp_avg_sq"):
                opt._check_tensor(st[name], name)
                if st[name].device != p.device or st[name].shape != p.shape:
                    raise LnsError("Stage2Trainer: optimizer state %s of %s does not match the parameter" % (name, k))
            for a, t in zip(arrs, (p, g, st["exp_avg"], st["exp_avg_sq"])):
                a[i] = t.data_ptr()
            params.append(p); grads.append(g); states.append(st)
        if len(params) != len(group["params"]) or len(opt.param_groups) != 1:
            raise LnsError("Stage2Trainer: the optimizer must hold exactly the propagator's parameters in one param group")
        dev = params[0].device
        self._params, self._grads, self._states = params, grads, states
        self._by_key = {k: p for _, k, p in table}
        self._steps = [st["step"] for st in states]
        self._arrs = arrs
        self._device = dev
        if self._loss is None or self._loss.device != dev:
            self._loss = torch.zeros(self._loss_ring, dtype=torch.float32, device=dev)
        self._key = self._signature()

    def _signature(self):
        return (_dropin._TREE_EPOCH[0], id(self.optimizer.state), tuple(p.data_ptr() for p in getattr(self, "_params", ())))

    def _current(self):
        if self._key is None or self._key != self._signature():
            self._resolve()
        # zero_grad(set_to_none=True) and user code may have dropped the buffers from .grad: they stay the gradient's home
        for p, g in zip(self._params, self._grads):
            if p.grad is not g:
                p.grad = g

    def set_wgrad(self, wgrad):
        """Weight-gradient kernel of the step: "tile" (one block per output tile) or "split" (batch-parallel); the engine's
        "train_wgrad" option.  Workspaces are kept per form, so switching on a live trainer allocates once per form."""
        if wgrad not in WGRAD_FORMS:
            raise LnsError("wgrad must be None, 'tile' or 'split', got %r" % (wgrad,))
        self._eng.set_option("train_wgrad", WGRAD_FORMS[wgrad])

    def _workspace(self, B, T, h, w, clip=False):
        # the size follows the engine's options ("train_wgrad"), however they were set: the library is asked (host-only) and
        # a workspace is only ever handed to the C call at the size it was allocated for
        need = (self._eng.train_step_clip_workspace_bytes if clip else self._eng.train_step_workspace_bytes)(B, h, w, T)
        key = (self._device, B, T, h, w, need, clip)
        ws = self._ws.get(key)
        if ws is None:
            with torch.cuda.device(self._device):
                ws = torch.empty(need, dtype=torch.uint8, device=self._device)
                if clip:
                    ws[-256:].zero_()          # the counter of skipped steps (include/lns.h: 256 bytes before the end)
            self._ws[key] = ws
        return ws

    @property
    def clipped(self):
        """Whether `step` goes through lns_train_step_clip (max_grad_norm, skip_nonfinite or an AdamW optimiser)."""
        return self.max_grad_norm is not None or self.skip_nonfinite or isinstance(self.optimizer, _optim.AdamW)

    @property
    def grad_norm(self):
        """Global L2 norm of the gradients before clipping, of the last clipped step: 0-dim view into a ring of `loss_ring`
        device floats (None before the first such step)."""
        return self._norm_last

    @property
    def skipped_steps(self):
        """Steps `skip_nonfinite` left out, as a 0-dim int32 device tensor (reading it synchronises; the step never does).
        One workspace (one batch shape): a view of its counter; several: their sum."""
        cs = [ws[-256:-252].view(torch.int32)[0] for key, ws in self._ws.items() if key[-1]]
        if not cs:
            return torch.zeros((), dtype=torch.int32, device=getattr(self, "_device", None))
        return cs[0] if len(cs) == 1 else torch.stack(cs).sum().to(torch.int32)

    # -- the step ------------------------------------------------------------------------------------------------------
    def step(self, z_in, z_out, param=None, update=True):
        """z_in [B,1,c,h,w], z_out [B,T,c,h,w] (fp32, on the parameters' device), param [B] for the conditional model.
        Returns the loss before the update as a 0-dim device tensor; never synchronises.  update=False: loss and
        gradients only (`.grad` is filled, unclipped; parameters and Adam state stay)."""
        self._current()
        if self.model._conditional != (param is not None):
            raise LnsError("param must be given exactly for the conditional model")
        if z_in.dim() != 5 or z_in.shape[1] != 1 or z_out.dim() != 5:
            raise LnsError("z_in must be [B,1,c,h,w] and z_out [B,T,c,h,w] (t_in == 1)")
        if z_in.device != self._device:
            raise LnsError("z_in is on %s but the propagator is on %s" % (z_in.device, self._device))
        B, _, _, h, w = z_in.shape
        T = int(z_out.shape[1])
        spec = None
        clip = update and self.clipped
        if update:
            t = {_optim._step_of(st) for st in self._states}
            if len(t) != 1:
                raise LnsError("Stage2Trainer: the propagator's parameters have different Adam step counts %s" % sorted(t))
            g = self.optimizer.param_groups[0]
            if clip:
                spec = _engine.update_spec(g["lr"], g["betas"], g["eps"], g["weight_decay"], t.pop() + 1, max_norm=self.max_grad_norm,
                                           decoupled=isinstance(self.optimizer, _optim.AdamW), skip_nonfinite=self.skip_nonfinite)
            else:
                spec = _engine.adam_spec(g["lr"], g["betas"], g["eps"], g["weight_decay"], t.pop() + 1)
        loss = self._loss[self._loss_i]
        if clip:
            if self._norm is None or self._norm.device != self._device:
                self._norm = torch.zeros(self._loss_ring, dtype=torch.float32, device=self._device)
            self._norm_last = self._norm[self._loss_i]
        self._loss_i = (self._loss_i + 1) % self._loss_ring
        a = self._arrs
        with torch.no_grad():
            if clip:
                self._eng.train_step_clip(a[0], z_in, z_out, a[1], a[2], a[3], spec, param=param, beta=self.beta, loss_out=loss,
                                          norm_out=self._norm_last, workspace=self._workspace(int(B), T, int(h), int(w), clip=True))
            else:
                self._eng.train_step(a[0], z_in, z_out, a[1], param=param, beta=self.beta, exp_avg=a[2], exp_avg_sq=a[3], spec=spec,
                                     loss_out=loss, workspace=self._workspace(int(B), T, int(h), int(w)))
            if update:
                torch._foreach_add_(self._steps, 1.0)
                # the kernel wrote the parameters through raw pointers: bump their versions, which is what
                # _Hosted._weights_signature (inference after training) and autograd watch
                for p in self._params:
                    torch._C._increment_version(p)
        return loss

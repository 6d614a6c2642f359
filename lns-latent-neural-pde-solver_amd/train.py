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
"""
import ctypes

import torch

from . import dropin as _dropin
from . import engine as _engine
from . import optim as _optim
from ._lib import LnsError

LOSS_RING = 4096
WGRAD_FORMS = {"tile": 0, "split": 1}


class Stage2Trainer:
    def __init__(self, model, optimizer=None, lr=1e-3, beta=1.0, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                 loss_ring=LOSS_RING, wgrad=None):
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
        self._key = None               # what the resolved pointers were taken from
        self._ws = {}                  # (device, B, T, h, w, bytes the engine asks for under its current options) -> workspace
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
        prefix = eng.cfg.prop_prefix.decode()
        named = dict(self._own.named_parameters())
        table = [(i, k, shape) for i, (k, shape, isb) in enumerate(eng.params) if k.startswith(prefix) and not isb]
        group = opt.param_groups[0]
        in_group = {id(p) for p in group["params"]}
        n = len(eng.params)
        arrs = [(ctypes.c_void_p * n)() for _ in range(4)]
        params, grads, states = [], [], []
        old = {id(p): g for p, g in zip(getattr(self, "_params", ()), getattr(self, "_grads", ()))}
        prev = getattr(self, "_by_key", {})
        for i, k, shape in table:
            p = named.get(k)
            if p is None:
                raise LnsError("Stage2Trainer: the model has no parameter %s" % k)
            if not p.is_cuda:
                raise LnsError("Stage2Trainer: parameter %s is on %s; the training step runs on HIP device tensors only "
                               "(call model.cuda()); there is no CPU fallback" % (k, p.device))
            if p.dtype != torch.float32 or not p.is_contiguous() or tuple(p.shape) != tuple(shape):
                raise LnsError("Stage2Trainer: %s must be a contiguous fp32 tensor of shape %s" % (k, tuple(shape)))
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
        if not params:
            raise LnsError("Stage2Trainer: the model has no propagator parameters")
        if len(params) != len(group["params"]) or len(opt.param_groups) != 1:
            raise LnsError("Stage2Trainer: the optimizer must hold exactly the propagator's parameters in one param group")
        dev = params[0].device
        if any(p.device != dev for p in params):
            raise LnsError("Stage2Trainer: the propagator's parameters live on several devices")
        self._params, self._grads, self._states = params, grads, states
        self._by_key = {k: named[k] for _, k, _ in table}
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

    def _workspace(self, B, T, h, w):
        # the size follows the engine's options ("train_wgrad"), however they were set: the library is asked (host-only) and
        # a workspace is only ever handed to the C call at the size it was allocated for
        need = self._eng.train_step_workspace_bytes(B, h, w, T)
        key = (self._device, B, T, h, w, need)
        ws = self._ws.get(key)
        if ws is None:
            with torch.cuda.device(self._device):
                ws = torch.empty(need, dtype=torch.uint8, device=self._device)
            self._ws[key] = ws
        return ws

    # -- the step ------------------------------------------------------------------------------------------------------
    def step(self, z_in, z_out, param=None, update=True):
        """z_in [B,1,c,h,w], z_out [B,T,c,h,w] (fp32, on the parameters' device), param [B] for the conditional model.
        Returns the loss before the update as a 0-dim device tensor; never synchronises.  update=False: loss and
        gradients only (`.grad` is filled, parameters and Adam state stay)."""
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
        if update:
            t = {_optim._step_of(st) for st in self._states}
            if len(t) != 1:
                raise LnsError("Stage2Trainer: the propagator's parameters have different Adam step counts %s" % sorted(t))
            g = self.optimizer.param_groups[0]
            spec = _engine.adam_spec(g["lr"], g["betas"], g["eps"], g["weight_decay"], t.pop() + 1)
        loss = self._loss[self._loss_i]
        self._loss_i = (self._loss_i + 1) % self._loss_ring
        a = self._arrs
        with torch.no_grad():
            self._eng.train_step(a[0], z_in, z_out, a[1], param=param, beta=self.beta, exp_avg=a[2], exp_avg_sq=a[3], spec=spec,
                                 loss_out=loss, workspace=self._workspace(int(B), T, int(h), int(w)))
            if update:
                torch._foreach_add_(self._steps, 1.0)
                # the kernel wrote the parameters through raw pointers: bump their versions, which is what
                # _Hosted._weights_signature (inference after training) and autograd watch
                for p in self._params:
                    torch._C._increment_version(p)
        return loss

"""`torch.optim.Adam` with the update on ONE HIP launch (lns_adam_step_tensors, csrc/lns_optim.inc).

Replaces `optim = torch.optim.Adam(propagator parameters, lr)` of the stage-2 scripts (train_stage2_ns2d.py:179) and its
`optim.step()` (:216).  It is a `torch.optim.Optimizer`: param groups, `zero_grad`, `CosineAnnealingLR` (:185, :227) and
`state_dict()` / `load_state_dict()` are the base class's, and the per-parameter state has torch's keys and dtypes
(`step`: fp32 host scalar tensor, `exp_avg`, `exp_avg_sq`: like the parameter), so a checkpoint written by either
optimiser (`optim_*.pt`, :203) resumes in the other.  Any fp32 contiguous HIP tensors, not only an engine's.  There is no
CPU path and none of the variants the kernel does not compute: amsgrad, maximize, capturable, sparse gradients raise.

`AdamW` is the same with torch.optim.AdamW's decoupled weight decay (lns_update_step_tensors) and torch.optim.AdamW's
state_dict layout; `clip_grad_norm_` is torch.nn.utils.clip_grad_norm_ (L2) on two kernels and a scale pass, returning the
norm as a device tensor without a read-back.  `lns_amd.train.Stage2Trainer` fuses both into its step.
"""
import ctypes

import torch

from . import _lib
from ._lib import LnsError


def _step_of(state):
    s = state["step"]
    return int(s.item()) if isinstance(s, torch.Tensor) else int(s)


class Adam(torch.optim.Optimizer):
    _DECOUPLED = False                     # AdamW below: the param group's `decoupled_weight_decay`, fixed by the class

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, maximize=False,
                 capturable=False, differentiable=False, foreach=None, fused=None, decoupled_weight_decay=False):
        if amsgrad or maximize or capturable or differentiable or decoupled_weight_decay:
            raise LnsError("lns_amd.optim.Adam computes plain Adam with L2 weight decay only: amsgrad / maximize / capturable / "
                           "differentiable / decoupled_weight_decay are not supported (use torch.optim.Adam)")
        if isinstance(lr, torch.Tensor):
            raise LnsError("lns_amd.optim.Adam: lr must be a Python number (it is a kernel argument; a tensor lr would need a read-back)")
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: %s" % lr)
        if not 0.0 < eps:
            raise ValueError("Invalid epsilon value: %s (the kernel needs eps > 0)" % eps)
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameters: %s" % (betas,))
        if not 0.0 <= weight_decay:
            raise ValueError("Invalid weight_decay value: %s" % weight_decay)
        # the keys torch.optim.Adam keeps in a param group, so that a state_dict moves between the two unchanged
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=self._DECOUPLED)
        super().__init__(params, defaults)

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:
            bad = [k for k in ("amsgrad", "maximize", "capturable", "differentiable") if group.get(k)]
            if self._DECOUPLED:
                # (a torch.optim.AdamW checkpoint from before the key existed has none: it means AdamW there)
                if not group.setdefault("decoupled_weight_decay", True):
                    raise LnsError("lns_amd.optim.AdamW: the loaded param group has decoupled_weight_decay=False, which is "
                                   "Adam with L2 weight decay: load it into lns_amd.optim.Adam")
            elif group.get("decoupled_weight_decay"):
                bad.append("decoupled_weight_decay")
            if bad:
                raise LnsError("lns_amd.optim.%s: the loaded param group asks for %s, which this optimiser does not compute"
                               % (type(self).__name__, " / ".join(bad)))
        for st in self.state.values():                 # checkpoints of old torch versions hold a Python number
            if "step" in st and not isinstance(st["step"], torch.Tensor):
                st["step"] = torch.tensor(float(st["step"]), dtype=torch.float32)

    @staticmethod
    def _check_tensor(p, what):
        if not p.is_cuda:
            raise LnsError("lns_amd.optim.Adam runs on HIP device tensors only (%s is on %s); there is no CPU fallback "
                           "-- use torch.optim.Adam on CPU" % (what, p.device))
        if p.is_sparse:
            raise LnsError("lns_amd.optim.Adam does not support sparse tensors (%s)" % what)
        if p.dtype != torch.float32 or not p.is_contiguous():
            raise LnsError("lns_amd.optim.Adam needs contiguous fp32 tensors (%s is %s, contiguous=%s)" % (what, p.dtype, p.is_contiguous()))

    def init_state(self, p):
        """torch.optim.Adam's lazily created state of one parameter."""
        st = self.state[p]
        if len(st) == 0:
            st["step"] = torch.tensor(0.0, dtype=torch.float32)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        L = _lib.lib()
        for group in self.param_groups:
            # tensors that share a step count (all of them, unless parameters joined later) go into one call
            by_step = {}
            for p in group["params"]:
                if p.grad is None or p.numel() == 0:
                    continue
                self._check_tensor(p, "a parameter")
                g = p.grad
                if g.is_sparse:
                    raise LnsError("lns_amd.optim.Adam does not support sparse gradients")
                self._check_tensor(g, "a gradient")
                st = self.init_state(p)
                self._check_tensor(st["exp_avg"], "exp_avg")
                self._check_tensor(st["exp_avg_sq"], "exp_avg_sq")
                by_step.setdefault((_step_of(st), p.device), []).append((p, g, st))
            for (t, dev), items in by_step.items():
                n = len(items)
                vp = ctypes.c_void_p * n
                tables = (vp(*[p.data_ptr() for p, _, _ in items]), vp(*[g.data_ptr() for _, g, _ in items]),
                          vp(*[st["exp_avg"].data_ptr() for _, _, st in items]),
                          vp(*[st["exp_avg_sq"].data_ptr() for _, _, st in items]),
                          (ctypes.c_int64 * n)(*[p.numel() for p, _, _ in items]))
                with torch.cuda.device(dev):
                    self._launch(L, n, tables, group, t + 1, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
                torch._foreach_add_([st["step"] for _, _, st in items], 1.0)
                # the kernel wrote through raw pointers: tell autograd and the drop-in's weight signature
                for p, _, st in items:
                    torch._C._increment_version(p)
        return loss

    @staticmethod
    def _launch(L, n, tables, group, step, stream):
        spec = _lib.LnsAdamSpec(ctypes.sizeof(_lib.LnsAdamSpec), 0, float(group["lr"]), float(group["betas"][0]),
                                float(group["betas"][1]), float(group["eps"]), float(group["weight_decay"]), step)
        rc = L.lns_adam_step_tensors(n, *tables, ctypes.byref(spec), stream)
        if rc != 0:
            raise LnsError("lns_adam_step_tensors failed (%d): %s" % (rc, L.lns_create_error().decode()))


class AdamW(Adam):
    """torch.optim.AdamW: `p *= 1 - lr * weight_decay`, then Adam on the gradient alone (lns_update_step_tensors with
    LNS_UPDATE_DECOUPLED_WD).  Param groups and state are torch.optim.AdamW's, so a state_dict moves between the two."""
    _DECOUPLED = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False,
                 foreach=None, capturable=False, differentiable=False, fused=None):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                         capturable=capturable, differentiable=differentiable, foreach=foreach, fused=fused)

    @staticmethod
    def _launch(L, n, tables, group, step, stream):
        from . import engine as _engine
        spec = _engine.update_spec(group["lr"], group["betas"], group["eps"], group["weight_decay"], step, decoupled=True)
        rc = L.lns_update_step_tensors(n, *tables, ctypes.byref(spec), None, stream)
        if rc != 0:
            raise LnsError("lns_update_step_tensors failed (%d): %s" % (rc, L.lns_create_error().decode()))


def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """torch.nn.utils.clip_grad_norm_ for fp32 HIP gradients: the global L2 norm in one launch set (double partials in a
    fixed order, lns_grad_norm_tensors), the coefficient min(1, max_norm / (norm + 1e-6)) on the device, one scale pass
    (lns_grad_scale_tensors).  Returns the norm before clipping as a 0-dim device tensor; never synchronises -- which is
    why error_if_nonfinite, whose answer the host would have to read, is refused, like every norm but L2.  With no
    gradient at all the result is a CPU `torch.tensor(0.0)`, which is what torch returns there too."""
    if float(norm_type) != 2.0:
        raise LnsError("lns_amd.optim.clip_grad_norm_ computes the L2 norm only (norm_type=%r): use torch.nn.utils.clip_grad_norm_" % (norm_type,))
    if error_if_nonfinite:
        raise LnsError("lns_amd.optim.clip_grad_norm_ does not read the norm back, so it cannot raise on a non-finite one")
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None and p.grad.numel() > 0]
    if not grads:
        return torch.tensor(0.0)
    dev = grads[0].device
    for g in grads:
        Adam._check_tensor(g, "a gradient")
        if g.device != dev:
            raise LnsError("lns_amd.optim.clip_grad_norm_: gradients live on several devices (%s, %s)" % (dev, g.device))
    L = _lib.lib()
    n = len(grads)
    ptrs = (ctypes.c_void_p * n)(*[g.data_ptr() for g in grads])
    numel = (ctypes.c_int64 * n)(*[g.numel() for g in grads])
    nbytes = ctypes.c_size_t(0)
    rc = L.lns_grad_norm_scratch_bytes(n, numel, ctypes.byref(nbytes))
    if rc == 0:
        with torch.cuda.device(dev):
            stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            scratch = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
            out = torch.empty(2, dtype=torch.float32, device=dev)             # norm, coefficient
            rc = L.lns_grad_norm_tensors(n, ptrs, numel, float(max_norm), out.data_ptr(), out.data_ptr() + 4, None, 0,
                                         scratch.data_ptr(), scratch.numel(), stream)
            if rc == 0:
                rc = L.lns_grad_scale_tensors(n, ptrs, numel, out.data_ptr() + 4, stream)
    if rc != 0:
        raise LnsError("lns_amd.optim.clip_grad_norm_ failed (%d): %s" % (rc, L.lns_create_error().decode()))
    return out[0]

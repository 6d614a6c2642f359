"""`torch.optim.Adam` with the update on ONE HIP launch (lns_adam_step_tensors, csrc/lns_optim.inc).

Replaces `optim = torch.optim.Adam(propagator parameters, lr)` of the stage-2 scripts (train_stage2_ns2d.py:179) and its
`optim.step()` (:216).  It is a `torch.optim.Optimizer`: param groups, `zero_grad`, `CosineAnnealingLR` (:185, :227) and
`state_dict()` / `load_state_dict()` are the base class's, and the per-parameter state has torch's keys and dtypes
(`step`: fp32 host scalar tensor, `exp_avg`, `exp_avg_sq`: like the parameter), so a checkpoint written by either
optimiser (`optim_*.pt`, :203) resumes in the other.  Any fp32 contiguous HIP tensors, not only an engine's.  There is no
CPU path and none of the variants the kernel does not compute: amsgrad, maximize, capturable, sparse gradients raise.
"""
import ctypes

import torch

from . import _lib
from ._lib import LnsError


def _step_of(state):
    s = state["step"]
    return int(s.item()) if isinstance(s, torch.Tensor) else int(s)


class Adam(torch.optim.Optimizer):
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
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False)
        super().__init__(params, defaults)

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:
            bad = [k for k in ("amsgrad", "maximize", "capturable", "differentiable", "decoupled_weight_decay") if group.get(k)]
            if bad:
                raise LnsError("lns_amd.optim.Adam: the loaded param group asks for %s, which this optimiser does not compute"
                               % " / ".join(bad))
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
                spec = _lib.LnsAdamSpec(ctypes.sizeof(_lib.LnsAdamSpec), 0, float(group["lr"]), float(group["betas"][0]),
                                        float(group["betas"][1]), float(group["eps"]), float(group["weight_decay"]), t + 1)
                with torch.cuda.device(dev):
                    rc = L.lns_adam_step_tensors(
                        n, vp(*[p.data_ptr() for p, _, _ in items]), vp(*[g.data_ptr() for _, g, _ in items]),
                        vp(*[st["exp_avg"].data_ptr() for _, _, st in items]),
                        vp(*[st["exp_avg_sq"].data_ptr() for _, _, st in items]),
                        (ctypes.c_int64 * n)(*[p.numel() for p, _, _ in items]), ctypes.byref(spec),
                        ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
                if rc != 0:
                    raise LnsError("lns_adam_step_tensors failed (%d): %s" % (rc, L.lns_create_error().decode()))
                torch._foreach_add_([st["step"] for _, _, st in items], 1.0)
                # the kernel wrote through raw pointers: tell autograd and the drop-in's weight signature
                for p, _, st in items:
                    torch._C._increment_version(p)
        return loss

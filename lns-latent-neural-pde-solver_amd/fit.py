"""`LatentFit`: the trained rollout run backwards onto data.

Two questions a differentiable surrogate is asked as soon as it is trained:

  * several observed frames, not one -- which initial latent z0 makes the rollout agree with all of them?
  * an unknown physical parameter -- which `param` of the conditional model explains an observed sequence?

Both are a descent on the inputs of the rollout with the propagator's weights held fixed.  One iteration is ONE call of the
C ABI (lns_fit_step): training forward over the steps up to the last observation, the observation loss (one loss per
trajectory: each sample is its own inverse problem)

    loss[b] = sum_k w_k mean((z_pred[b, t_k] - obs[b, k])^2) + background * mean((z0[b] - z_background[b])^2),

the state-only adjoint of the rollout (no weight, bias or affine gradient is computed) down to z0 and, through the vector
network and the Fourier embedding, to `param`, then Adam on z0 and on `param`, each with its own learning rate.  Nothing in
the loop synchronises, allocates or copies from the host: the propagator's parameter pointers are resolved once (by the rule
`lns_amd.train.Stage2Trainer` uses, and again only when that rule says they moved), and one workspace is kept per shape.

No reference counterpart: the reference trains the propagator and never fits its inputs.
"""
import ctypes

import torch

from . import dropin as _dropin
from . import engine as _engine
from . import train as _train
from ._lib import LnsError


class FitResult(tuple):
    """(z0, param, loss, per): the fitted initial latent [B,c,h,w], the fitted (or given) param [B] or None, the loss of
    every iteration BEFORE its update [iters, B] and the last iteration's per-observation mean squared errors [B, n_obs]."""
    __slots__ = ()
    z0 = property(lambda s: s[0])
    param = property(lambda s: s[1])
    loss = property(lambda s: s[2])
    per = property(lambda s: s[3])


class LatentFit:
    def __init__(self, model, lr_state=2e-3, lr_param=1e-2, betas=(0.9, 0.999), eps=1e-8, background=0.0, fit_state=True,
                 fit_param=None):
        if not isinstance(model, _dropin.LatentDynamics):
            raise LnsError("LatentFit needs a LatentDynamics drop-in (lns_amd.dropin), got %s" % type(model).__name__)
        self.model = model
        self._own = model._owner
        self._eng = self._own._eng
        self.fit_state = bool(fit_state)
        self.fit_param = model._conditional if fit_param is None else bool(fit_param)     # None: "the model is conditional"
        if self.fit_param and not model._conditional:
            raise LnsError("fit_param needs the conditional model: a plain propagator has no param")
        if not self.fit_state and not self.fit_param:
            raise LnsError("nothing to fit: fit_state and fit_param are both off")
        if not float(background) >= 0:
            raise LnsError("background must be >= 0, got %r" % (background,))
        self.lr_state, self.lr_param = float(lr_state), float(lr_param)
        self.betas, self.eps, self.background = (float(betas[0]), float(betas[1])), float(eps), float(background)
        self._key = None
        self._ws = {}                  # (device, B, h, w, T, n_obs, bytes the engine asks for) -> workspace

    def _signature(self):
        return (_dropin._TREE_EPOCH[0], tuple(p.data_ptr() for p in getattr(self, "_params", ())))

    def _current(self):
        if self._key is None or self._key != self._signature():
            table = _train.propagator_tensors(self._own, self._eng, who="LatentFit")
            arr = (ctypes.c_void_p * len(self._eng.params))()
            for i, _, p in table:
                arr[i] = p.data_ptr()
            self._params = [p for _, _, p in table]
            self._arr = arr
            self._device = self._params[0].device
            self._key = self._signature()

    def _workspace(self, B, h, w, T, n_obs):
        need = self._eng.fit_step_workspace_bytes(B, h, w, T, n_obs)
        key = (self._device, B, h, w, T, n_obs, need)
        ws = self._ws.get(key)
        if ws is None:
            with torch.cuda.device(self._device):
                ws = torch.empty(need, dtype=torch.uint8, device=self._device)
            self._ws[key] = ws
        return ws

    @torch.no_grad()
    def run(self, z0, obs, obs_steps, param=None, weights=None, iters=40, z_background=None):
        """z0 [B,c,h,w]: the start (and, with background > 0, the background unless z_background is given); obs
        [B,n_obs,c,h,w]: the observed latents at the 0-based rollout steps `obs_steps` (step t is the rollout's t-th output:
        step 0 is one propagator application after z0); param [B]: the start of the fitted parameter, or its known value;
        weights: one per observation (None: all 1).  Returns FitResult(z0, param, loss [iters, B], per [B, n_obs]) -- device
        tensors, never read back here.  The caller's z0 / param keep their values: the fit works on clones."""
        self._current()
        iters = int(iters)
        if iters < 1:
            raise LnsError("iters must be >= 1")
        if self.model._conditional != (param is not None):
            raise LnsError("param must be given exactly for the conditional model")
        if not isinstance(z0, torch.Tensor) or z0.dim() != 4 or z0.device != self._device:
            raise LnsError("z0 must be [B,c,h,w] on the propagator's device %s" % (self._device,))
        steps, w_ = _engine.normalize_obs(obs_steps, weights)
        with torch.cuda.device(self._device):
            z = z0.detach().to(torch.float32).clone(memory_format=torch.contiguous_format)
            B, c, h, w = z.shape
            p = None
            if param is not None:
                p = self._eng._param(param, z).clone()
            zb = None
            if self.background > 0 or z_background is not None:
                zb = (z0 if z_background is None else z_background).detach().to(torch.float32).clone(memory_format=torch.contiguous_format)
            dev = self._device
            gz = mz = vz = gp = mp = vp = None
            if self.fit_state:
                gz, mz, vz = torch.zeros_like(z), torch.zeros_like(z), torch.zeros_like(z)
            if self.fit_param:
                gp, mp, vp = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
            loss = torch.empty((iters, B), dtype=torch.float32, device=dev)
            per = torch.empty((B, len(steps)), dtype=torch.float32, device=dev)
            ws = self._workspace(B, h, w, steps[-1] + 1, len(steps))
            obs = self._eng._dev(obs)
            for it in range(iters):
                spec = _engine.fit_spec(
                    steps, w_, self.background,
                    state=_engine.update_spec(self.lr_state, self.betas, self.eps, step=it + 1) if self.fit_state else None,
                    param=_engine.update_spec(self.lr_param, self.betas, self.eps, step=it + 1) if self.fit_param else None)
                self._eng.fit_step(self._arr, z, obs, spec, param=p, z_background=zb, g_z=gz, exp_avg_z=mz, exp_avg_sq_z=vz, g_p=gp,
                                   exp_avg_p=mp, exp_avg_sq_p=vp, loss=loss[it], per=per, workspace=ws)
        return FitResult((z, p, loss, per))

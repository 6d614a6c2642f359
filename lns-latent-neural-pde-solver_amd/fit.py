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
        self._param_fit_asked = fit_param is not None and bool(fit_param)                 # run_gauss_newton refuses only this
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

    def _gn_workspace(self, B, h, w, T, n_obs):
        need = self._eng.fit_gn_step_workspace_bytes(B, h, w, T, n_obs)
        key = ("gn", self._device, B, h, w, T, n_obs, need)
        ws = self._ws.get(key)
        if ws is None:
            with torch.cuda.device(self._device):
                ws = torch.empty(need, dtype=torch.uint8, device=self._device)
            self._ws[key] = ws
        return ws

    def _start(self, z0, param):
        """What run and the Gauss-Newton calls refuse about (z0, param), and the pointer table."""
        self._current()
        if self.model._conditional != (param is not None):
            raise LnsError("param must be given exactly for the conditional model")
        if not isinstance(z0, torch.Tensor) or z0.dim() != 4 or z0.device != self._device:
            raise LnsError("z0 must be [B,c,h,w] on the propagator's device %s" % (self._device,))

    @torch.no_grad()
    def run_gauss_newton(self, z0, obs, obs_steps, param=None, weights=None, outer=3, cg_iters=8, damping=0.0, cg_tol=0.0,
                         z_background=None):
        """The fit of the STATE by Gauss-Newton: `outer` iterations, each ONE call of the C ABI (lns_fit_gn_step) -- forward,
        observation loss, state-only adjoint, `cg_iters` steps of conjugate gradients on H delta = -g with H v from the
        tangent-linear rollout and the adjoint, z0 += delta.  damping: Levenberg's mu added to the diagonal of H (absolute);
        cg_tol: a sample's CG stops at |r| <= cg_tol |r0|.  No line search: the step is taken as it is.  param [B]: the known
        parameter of the conditional model (the tangent has no param direction, so it is not fitted here: an instance built
        with fit_param=True is refused).  Arguments otherwise as in `run`.  Returns FitResult(z0, param, loss [outer + 1, B],
        per [B, n_obs]): row i < outer is the loss before iteration i, the last row the loss of the returned z0 (one more
        forward and observation loss), per belongs to it.  Works on clones; never synchronises."""
        if self._param_fit_asked:
            raise LnsError("run_gauss_newton fits the state only: the tangent-linear rollout has no param direction, so there "
                           "is no Gauss-Newton product for param; build LatentFit without fit_param=True (param is then a "
                           "known input), or use run")
        self._start(z0, param)
        outer = int(outer)
        if outer < 1:
            raise LnsError("outer must be >= 1")
        steps, w_ = _engine.normalize_obs(obs_steps, weights)
        with torch.cuda.device(self._device):
            z = z0.detach().to(torch.float32).clone(memory_format=torch.contiguous_format)
            B, c, h, w = z.shape
            p = self._eng._param(param, z).clone() if param is not None else None
            zb = None
            if self.background > 0 or z_background is not None:
                zb = (z0 if z_background is None else z_background).detach().to(torch.float32).clone(memory_format=torch.contiguous_format)
            dev = self._device
            T = steps[-1] + 1
            loss = torch.empty((outer + 1, B), dtype=torch.float32, device=dev)
            per = torch.empty((B, len(steps)), dtype=torch.float32, device=dev)
            resid = torch.empty(B, dtype=torch.float32, device=dev)
            applied = torch.empty(B, dtype=torch.int32, device=dev)
            ws = self._gn_workspace(B, h, w, T, len(steps))
            obs = self._eng._dev(obs)
            spec = _engine.gn_spec(steps, w_, self.background, n_cg=cg_iters, damping=damping, cg_tol=cg_tol)
            for it in range(outer):
                self._eng.fit_gn_step(self._arr, z, obs, spec, param=p, z_background=zb, loss=loss[it], per=per, cg_resid=resid,
                                      applied=applied, workspace=ws)
            z_pred, _ = self._eng.train_forward(self._arr, z, T, param=p, workspace=ws)
            bg = dict(z0=z, z_background=zb, background=self.background, need_bg_grad=False) if zb is not None else {}
            last, per, _, _ = _engine.obs_loss(z_pred, obs, steps, w_, **bg)
            loss[outer].copy_(last)
        return FitResult((z, p, loss, per))

    @torch.no_grad()
    def hessian_product(self, z0, v, obs_steps, param=None, weights=None, damping=0.0):
        """(H v, v^T H v) of the Gauss-Newton operator of the fit's loss at z0 for every vector of v [B,K,c,h,w]: one training
        forward, then one lns_train_gn_product per k.  Returns (hv [B,K,c,h,w], vhv [B,K] float64); uses self.background."""
        self._start(z0, param)
        steps, w_ = _engine.normalize_obs(obs_steps, weights)
        if not isinstance(v, torch.Tensor) or v.dim() != 5 or v.shape[0] != z0.shape[0] or v.shape[2:] != z0.shape[1:] or v.device != z0.device:
            raise LnsError("v must be [B,K,c,h,w] matching z0 %s on its device" % (tuple(z0.shape),))
        with torch.cuda.device(self._device):
            z = self._eng._dev(z0.detach())
            B, c, h, w = z.shape
            K, T = int(v.shape[1]), steps[-1] + 1
            p = self._eng._param(param, z) if param is not None else None
            ws = self._gn_workspace(B, h, w, T, len(steps))
            z_pred, _ = self._eng.train_forward(self._arr, z, T, param=p, workspace=ws)
            hv = torch.empty((K, B, c, h, w), dtype=torch.float32, device=self._device)
            vhv = torch.empty((K, B), dtype=torch.float64, device=self._device)
            vk = v.detach().to(torch.float32).transpose(0, 1).contiguous()
            for k in range(K):
                self._eng.train_gn_product(self._arr, z, z_pred, vk[k], steps, ws, weights=w_, background=self.background,
                                           damping=damping, hv=hv[k], vhv=vhv[k])
        return hv.transpose(0, 1).contiguous(), vhv.transpose(0, 1).contiguous()

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

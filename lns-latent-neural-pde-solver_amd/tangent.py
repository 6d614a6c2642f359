"""`TangentRollout`: perturbations of the initial latent carried forward along a trajectory of the trained rollout.

`LatentFit` runs the rollout backwards (J^T w: the state-only adjoint); this is the forward half, J v (lns_train_tangent):
K tangents of every sample ride the batch axis through the propagator's steps, against the tape of one training forward.
Differencing two nonlinear rollouts instead loses about half of the fp32 digits and costs a rollout per direction.

  * `jvp(z0, v, T)`: the rollout and the tangents after every (kept) step -- one forward, one tangent call;
  * `lyapunov(z0, T, k)`: the Benettin loop -- k tangents, re-orthonormalised every `renorm` steps by modified Gram-Schmidt
    (lns_op_orthonormalize, sums in double), the logarithms of the stretching factors R_kk accumulated on the device.  The
    exponents' inverse is the e-folding time of a perturbation; the orthonormal basis the run ends with spans the growing
    directions at the last latent (an ensemble perturbed along them adds `amp * vectors[:, j]` to that latent).

Nothing in either loop synchronises or reads back; the propagator's parameter pointers are resolved by the rule
`Stage2Trainer` and `LatentFit` use, and one workspace is kept per shape.

No reference counterpart: the reference never linearises its propagator.
"""
import ctypes

import torch

from . import _lib
from . import dropin as _dropin
from . import train as _train
from ._lib import LnsError


class LyapunovResult(tuple):
    """(exponents, history, vectors, z_last): the finite-time Lyapunov exponents [B,k] float64 (per unit of `dt`), log R_kk of
    every accumulated re-orthonormalisation [n_renorm,B,k] float64, the orthonormal tangents at the last latent [B,k,c,h,w]
    and that latent [B,c,h,w]."""
    __slots__ = ()
    exponents = property(lambda s: s[0])
    history = property(lambda s: s[1])
    vectors = property(lambda s: s[2])
    z_last = property(lambda s: s[3])


class TangentRollout:
    def __init__(self, model):
        if not isinstance(model, _dropin.LatentDynamics):
            raise LnsError("TangentRollout needs a LatentDynamics drop-in (lns_amd.dropin), got %s" % type(model).__name__)
        self.model = model
        self._own = model._owner
        self._eng = self._own._eng
        self._key = None
        self._ws = {}                  # (device, B, h, w, T, K, bytes the engine asks for) -> workspace

    def _signature(self):
        return (_dropin._TREE_EPOCH[0], tuple(p.data_ptr() for p in getattr(self, "_params", ())))

    def _current(self):
        if self._key is None or self._key != self._signature():
            table = _train.propagator_tensors(self._own, self._eng, who="TangentRollout")
            arr = (ctypes.c_void_p * len(self._eng.params))()
            for i, _, p in table:
                arr[i] = p.data_ptr()
            self._params = [p for _, _, p in table]
            self._arr = arr
            self._device = self._params[0].device
            self._key = self._signature()

    def _workspace(self, B, h, w, T, K):
        need = self._eng.train_tangent_workspace_bytes(B, h, w, T, K)
        key = (self._device, B, h, w, T, K, need)
        ws = self._ws.get(key)
        if ws is None:
            with torch.cuda.device(self._device):
                ws = torch.empty(need, dtype=torch.uint8, device=self._device)
            self._ws[key] = ws
        return ws

    def _start(self, z0, param):
        self._current()
        if self.model._conditional != (param is not None):
            raise LnsError("param must be given exactly for the conditional model")
        if not isinstance(z0, torch.Tensor) or z0.dim() != 4 or z0.device != self._device:
            raise LnsError("z0 must be [B,c,h,w] on the propagator's device %s" % (self._device,))
        z = self._eng._dev(z0.detach())
        return z, (self._eng._param(param, z) if param is not None else None)

    @torch.no_grad()
    def jvp(self, z0, v, T, param=None, keep_steps=None):
        """z0 [B,c,h,w]; v [B,K,c,h,w] or [B,c,h,w] (K = 1): perturbations of z0, left unchanged.  Returns (z_pred
        [B,T,c,h,w], jv [B,K,n_keep,c,h,w]): the rollout and J v after the 0-based steps `keep_steps` (None: every step;
        step t is the rollout's t-th output).  Device tensors, never read back here."""
        T = int(T)
        if T < 1:
            raise LnsError("T must be >= 1")
        z, p = self._start(z0, param)
        if not isinstance(v, torch.Tensor) or v.dim() not in (4, 5) or v.shape[0] != z.shape[0] or v.shape[-3:] != z.shape[1:] \
                or v.device != z.device or v.dtype != torch.float32:
            raise LnsError("v must be fp32 [B,K,c,h,w] or [B,c,h,w] matching z0 %s on its device" % (tuple(z.shape),))
        keep = None
        if keep_steps is not None:
            keep = [int(t) for t in keep_steps]
            if not keep or any(t < 0 or t >= T for t in keep):
                raise LnsError("keep_steps must be 0-based steps below T = %d" % T)
        B, c, h, w = z.shape
        with torch.cuda.device(self._device):
            vv = (v[:, None] if v.dim() == 4 else v).detach().clone(memory_format=torch.contiguous_format)
            K = int(vv.shape[1])
            ws = self._workspace(B, h, w, T, K)
            z_pred, _ = self._eng.train_forward(self._arr, z, T, param=p, workspace=ws)
            jv = self._eng.train_tangent(self._arr, vv, T, ws, keep=True)
            if keep is not None:
                jv = jv[:, :, keep]
        return z_pred, jv

    @torch.no_grad()
    def lyapunov(self, z0, T, k=4, renorm=1, burn_in=0, chunk=None, param=None, generator=None, dt=1.0):
        """The k leading finite-time Lyapunov exponents of the rollout started at z0 [B,c,h,w], over T steps (Benettin):
        k tangents start as normals from `generator`, orthonormalised; they are carried through the steps and
        re-orthonormalised every `renorm` steps, log R_kk accumulating after the first `burn_in` steps:
        exponents = sum log R_kk / ((T - burn_in) * dt).  T - burn_in must be a positive multiple of renorm (the
        re-orthonormalisations are at the steps t with (T - t) % renorm == 0).  chunk: steps per training forward (the
        tape of `chunk` steps is held; None: all T); the result does not depend on it."""
        T, k, renorm, burn_in = int(T), int(k), int(renorm), int(burn_in)
        if T < 1 or renorm < 1 or burn_in < 0:
            raise LnsError("lyapunov: T >= 1, renorm >= 1 and burn_in >= 0, got T %d, renorm %d, burn_in %d" % (T, renorm, burn_in))
        if k < 1 or k > _lib.LNS_TANGENT_MAX:
            raise LnsError("lyapunov: k must be in 1 .. %d, got %d" % (_lib.LNS_TANGENT_MAX, k))
        if T - burn_in < 1 or (T - burn_in) % renorm != 0:
            raise LnsError("lyapunov: T - burn_in must be a positive multiple of renorm, got T %d, burn_in %d, renorm %d" % (T, burn_in, renorm))
        chunk = T if chunk is None else int(chunk)
        if chunk < 1:
            raise LnsError("lyapunov: chunk must be >= 1")
        if not float(dt) > 0:
            raise LnsError("lyapunov: dt must be > 0")
        z, p = self._start(z0, param)
        B, c, h, w = z.shape
        if k > c * h * w:
            raise LnsError("lyapunov: k = %d tangents do not fit a latent of %d numbers" % (k, c * h * w))
        n_renorm = (T - burn_in) // renorm
        eng = self._eng
        with torch.cuda.device(self._device):
            dev = self._device
            V = torch.randn((B, k, c, h, w), dtype=torch.float32, device=dev, generator=generator)
            eng.orthonormalize(V)
            logr = torch.zeros((B, k), dtype=torch.float64, device=dev)
            R = torch.empty((B, k, k), dtype=torch.float64, device=dev)
            history = torch.empty((n_renorm, B, k), dtype=torch.float64, device=dev)
            row = 0
            for c0 in range(0, T, chunk):
                Tc = min(chunk, T - c0)
                ws = self._workspace(B, h, w, Tc, k)
                z_pred, _ = eng.train_forward(self._arr, z, Tc, param=p, workspace=ws)
                t = c0
                while t < c0 + Tc:
                    stop = min(c0 + Tc, t + 1 + (T - t - 1) % renorm)        # the next re-orthonormalisation, or the chunk's end
                    eng.train_tangent(self._arr, V, Tc, ws, t0=t - c0, nsteps=stop - t)
                    t = stop
                    if (T - t) % renorm == 0:
                        if t > burn_in:
                            eng.orthonormalize(V, r_out=R, logr_acc=logr)
                            history[row] = torch.log(torch.diagonal(R, dim1=1, dim2=2))
                            row += 1
                        else:
                            eng.orthonormalize(V)
                z = z_pred[:, Tc - 1].contiguous()
            exponents = logr / ((T - burn_in) * float(dt))
        return LyapunovResult((exponents, history, V, z))

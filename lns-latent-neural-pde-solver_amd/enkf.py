"""`EnsembleFilter`: an ensemble of latents corrected by sparse observations of the decoded fields.

`LatentDynamics.assimilate` fits a latent to data by encoding the observed frames: it needs complete frames of every channel.
A surrogate is more often asked to take in a few sensors, one observed channel or a masked region.  The ensemble transform
Kalman filter (ETKF; Hunt, Kostelich, Szunyogh 2007, without localisation) does that without an adjoint of anything: the
members are rolled out, decoded at the observed steps and compared with the observations in physical space, and the M x M
transform that the comparison gives is applied to the LATENT members -- and to a per-member `param`, so a parameter of a
conditional model is estimated from sparse decoded observations as well.

One window is ONE call of the C ABI (lns_rollout_latent_ensemble_analysis; the statement and the order of every sum:
include/lns.h): per sample, with Y the members' decoded anomalies at the observed values, r the inverse observation-error
variances and d the innovation of the ensemble mean,

    S = Y^T diag(r) Y,  g = Y^T diag(r) d,  A = (M - 1) / rho I + S = Q Lambda Q^T,
    wbar = Q Lambda^-1 Q^T g,  W = sqrt(M - 1) Q Lambda^-1/2 Q^T,  X = W + wbar 1^T,
    z_analysis_m = zbar + sum_k (z_k - zbar) X_km

with the observations of all the steps of a window summed into one S and g (the 4D form).  Nothing in a cycle of windows
synchronises or reads back.

`LocalEnsembleFilter` is the localised form (the local ETKF of the same paper; lns_rollout_latent_ensemble_analysis_local): the
decoded frame is cut into the h x w patches of the latent grid, the Gram sums are taken per patch, and latent pixel l gets its
own transform from the patch sums weighted by the Gaspari-Cohn taper of the distance in latent pixels (`gaspari_cohn`,
`localization_weights`: the statement's taper on the host, float64).  A per-member `param` is not spatial and keeps the global
transform.

Not there: more than 64 members, additive inflation, correlated observation errors, observation operators that are not
pointwise in the decoded frame, domains other than one latent pixel, tapers other than Gaspari-Cohn.  No reference
counterpart: the reference never assimilates.
"""
import collections

import numpy as np
import torch

from ._lib import LnsError

EnKFResult = collections.namedtuple("EnKFResult", "z param X lam stat status dfs")
EnKFResult.__doc__ = """Result of EnsembleFilter.analysis / run over n_win windows: z [B, M, c, h, w] the analysis latents at the last
observed step, param [B, M] the analysis of a per-member param (else what was given, or None), X [n_win, B, M, M] and lam
[n_win, B, M] (float64; the eigenvalues of (M-1)/rho I + S, ascending), stat [B, n_obs, 3] (float64: the forecast mean's
weighted misfit sum r d^2, sum r and the number of observed values per observed step), status [n_win, B] (int32: 0 ok, 1
non-finite Gram, 2 not converged) and dfs [n_win, B] = sum_i (1 - (M-1) / (rho lam_i)), the degrees of freedom for signal
(between 0: the observations changed nothing, and min(M - 1, number of observed values))."""


class EnsembleFilter:
    """EnsembleFilter(model, inflation=1.0): the ETKF on the rollout of a `LatentDynamics` (or an object with `_engine(like)`).
    inflation: the multiplicative inflation rho >= 1 of the forecast anomalies."""

    def __init__(self, model, inflation=1.0):
        rho = float(inflation)
        if not rho >= 1.0 or rho == float("inf"):
            raise LnsError("inflation must be finite and >= 1, got %r" % (inflation,))
        self.model = model
        self.rho = rho

    def dfs(self, lam, members):
        """sum_i (1 - (M-1) / (rho lam_i)) over the last axis, on lam's device"""
        return (1.0 - (members - 1) / (self.rho * lam)).sum(-1)

    def _window(self, z, y_obs, rinv, steps, keep, param, norm):
        eng = self.model._engine(z)
        return eng.rollout_latent_ensemble_analysis(z, y_obs, rinv, steps, param=param, keep_steps=keep, rho=self.rho, **norm)

    @torch.no_grad()
    def analysis(self, z, y_obs, rinv, steps, obs_steps, param=None, **norm):
        """One window: z [B, M, c, h, w] rolled `steps` steps, the observations y_obs [B, n_obs, C, Ly, Lx] of the steps
        `obs_steps` (ascending, in [0, steps); step 0 is one propagator step after z) weighted by rinv ([C, Ly, Lx],
        [n_obs, C, Ly, Lx] or [B, n_obs, C, Ly, Lx]; 0: not observed) -> EnKFResult whose z are the latents of step
        `steps - 1` after the analysis.  `norm` as in `validate`: the units rinv is given in."""
        keep = [int(s) for s in obs_steps]
        a = self._window(z, y_obs, rinv, int(steps), keep, param, norm)
        M = int(z.shape[1])
        return EnKFResult(a.z, a.param if a.param is not None else param, a.X[None], a.lam[None], a.stat, a.status[None],
                          self.dfs(a.lam, M)[None])

    @torch.no_grad()
    def run(self, z, y_obs, rinv, obs_steps, window=1, param=None, **norm):
        """Cycle over windows of `window` observations: window w rolls from the previous analysis (the first from z) to its
        last observed step, takes in its observations at once and hands its analysis on.  obs_steps: ascending steps, step 0
        one propagator step after z.  Returns EnKFResult with one X / lam / status / dfs per window; its z are the latents
        at the last observed step.  Nothing is read back."""
        obs = [int(s) for s in obs_steps]
        window = int(window)
        if window < 1:
            raise LnsError("window must be at least 1, got %d" % window)
        if not obs or any(b <= a for a, b in zip(obs, obs[1:])) or obs[0] < 0:
            raise LnsError("obs_steps must be ascending steps >= 0, got %s" % (obs,))
        n_obs = len(obs)
        if y_obs.dim() != 5 or y_obs.shape[1] != n_obs:
            raise LnsError("y_obs must be [B, %d, C, Ly, Lx] for %d observed steps, got %s" % (n_obs, n_obs, tuple(y_obs.shape)))
        per_step = rinv.dim() >= 4
        M = int(z.shape[1])
        Xs, lams, stats, statuses = [], [], [], []
        start = 0                                      # the step the window's first propagator step produces
        for k0 in range(0, n_obs, window):
            steps_w = obs[k0:k0 + window]
            T = steps_w[-1] - start + 1
            r_w = rinv[..., k0:k0 + window, :, :, :] if per_step else rinv
            a = self._window(z, y_obs[:, k0:k0 + window], r_w, T, [s - start for s in steps_w], param, norm)
            z = a.z
            if a.param is not None:
                param = a.param
            Xs.append(a.X)
            lams.append(a.lam)
            stats.append(a.stat)
            statuses.append(a.status)
            start = steps_w[-1] + 1
        lam = torch.stack(lams)
        return EnKFResult(z, param, torch.stack(Xs), lam, torch.cat(stats, 1), torch.stack(statuses), self.dfs(lam, M))


# ---- the localised filter ----------------------------------------------------------------------------------------------------
LocalEnKFResult = collections.namedtuple("LocalEnKFResult", "z param X lam stat status dfs")
LocalEnKFResult.__doc__ = """Result of LocalEnsembleFilter.analysis / run over n_win windows: z, param and stat as EnKFResult (param by
the global transform); per domain lam [n_win, B, h*w, M], status [n_win, B, h*w] and dfs [n_win, B, h*w] (the degrees of freedom
for signal of latent pixel l's local problem); X [n_win, B, h*w, M, M], or None with keep_X = False."""


def gaspari_cohn(r):
    """The Gaspari-Cohn taper of include/lns.h at r = distance / half-width >= 0, in float64 and in the statement's order (the
    device's bits): 1 at 0, 5/24 at 1, 0 from 2 on."""
    r = np.asarray(r, dtype=np.float64)
    one, c53, c58, c112 = np.float64(1.0), np.float64(5.0) / np.float64(3.0), np.float64(5.0) / np.float64(8.0), \
        np.float64(1.0) / np.float64(12.0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):      # (both branches are evaluated everywhere)
        r2 = r * r
        r3 = r2 * r
        r4 = r3 * r
        r5 = r4 * r
        near = (((one - c53 * r2) + c58 * r3) + np.float64(0.5) * r4) - np.float64(0.25) * r5
        far = (((((np.float64(4.0) - np.float64(5.0) * r) + c53 * r2) + c58 * r3) - np.float64(0.5) * r4) + c112 * r5) \
            - np.float64(2.0) / (np.float64(3.0) * r)
    far = np.where(far > 0.0, far, 0.0)
    return np.where(r >= 2.0, 0.0, np.where(r <= 1.0, near, far))


def localization_weights(h, w, radius, boundary):
    """rho [h*w, h*w] float64: the weight of patch t in the local domain of latent pixel l on an h x w grid, radius the half-width
    in latent pixels; boundary: "periodic", "wall" or a pair (y, x) (metrics.flow_boundary; the distance wraps on a periodic axis)."""
    from . import metrics
    bc_y, bc_x = metrics.flow_boundary(boundary)
    radius = float(radius)
    if not radius > 0.0 or radius == float("inf"):
        raise LnsError("radius must be finite and > 0, got %r" % (radius,))
    i, j = np.divmod(np.arange(h * w), w)
    dy = np.abs(i[:, None] - i[None, :])
    dx = np.abs(j[:, None] - j[None, :])
    if bc_y == 0:
        dy = np.minimum(dy, h - dy)
    if bc_x == 0:
        dx = np.minimum(dx, w - dx)
    dist = np.sqrt((dy * dy + dx * dx).astype(np.float64))
    return gaspari_cohn(dist / np.float64(radius))


class LocalEnsembleFilter(EnsembleFilter):
    """LocalEnsembleFilter(model, loc_radius, inflation=1.0, boundary="auto"): EnsembleFilter with one transform per latent pixel.
    loc_radius: the Gaspari-Cohn half-width in latent pixels; boundary: as metrics.flow_boundary ("auto": the model's padding per
    axis); keep_X = False drops the [B, h*w, M, M] transforms from the result."""

    def __init__(self, model, loc_radius, inflation=1.0, boundary="auto", keep_X=True):
        super().__init__(model, inflation)
        radius = float(loc_radius)
        if not radius > 0.0 or radius == float("inf"):
            raise LnsError("loc_radius must be finite and > 0, got %r" % (loc_radius,))
        self.loc_radius = radius
        self.boundary = boundary
        self.keep_X = bool(keep_X)

    def _window(self, z, y_obs, rinv, steps, keep, param, norm):
        eng = self.model._engine(z)
        return eng.rollout_latent_ensemble_analysis_local(z, y_obs, rinv, steps, self.loc_radius, boundary=self.boundary, param=param,
                                                          keep_steps=keep, rho=self.rho, return_X=self.keep_X, **norm)

    @torch.no_grad()
    def analysis(self, z, y_obs, rinv, steps, obs_steps, param=None, **norm):
        """One window, as EnsembleFilter.analysis -> LocalEnKFResult"""
        keep = [int(s) for s in obs_steps]
        a = self._window(z, y_obs, rinv, int(steps), keep, param, norm)
        M = int(z.shape[1])
        return LocalEnKFResult(a.z, a.param if a.param is not None else param, a.X_local[None] if self.keep_X else None, a.lam_local[None],
                               a.stat, a.status_local[None], self.dfs(a.lam_local, M)[None])

    @torch.no_grad()
    def run(self, z, y_obs, rinv, obs_steps, window=1, param=None, **norm):
        """Cycle over windows, as EnsembleFilter.run -> LocalEnKFResult with one lam / status / dfs (and X) per window and domain"""
        obs = [int(s) for s in obs_steps]
        window = int(window)
        if window < 1:
            raise LnsError("window must be at least 1, got %d" % window)
        if not obs or any(b <= a for a, b in zip(obs, obs[1:])) or obs[0] < 0:
            raise LnsError("obs_steps must be ascending steps >= 0, got %s" % (obs,))
        n_obs = len(obs)
        if y_obs.dim() != 5 or y_obs.shape[1] != n_obs:
            raise LnsError("y_obs must be [B, %d, C, Ly, Lx] for %d observed steps, got %s" % (n_obs, n_obs, tuple(y_obs.shape)))
        per_step = rinv.dim() >= 4
        M = int(z.shape[1])
        Xs, lams, stats, statuses = [], [], [], []
        start = 0
        for k0 in range(0, n_obs, window):
            steps_w = obs[k0:k0 + window]
            T = steps_w[-1] - start + 1
            r_w = rinv[..., k0:k0 + window, :, :, :] if per_step else rinv
            a = self._window(z, y_obs[:, k0:k0 + window], r_w, T, [s - start for s in steps_w], param, norm)
            z = a.z
            if a.param is not None:
                param = a.param
            Xs.append(a.X_local)
            lams.append(a.lam_local)
            stats.append(a.stat)
            statuses.append(a.status_local)
            start = steps_w[-1] + 1
        lam = torch.stack(lams)
        return LocalEnKFResult(z, param, torch.stack(Xs) if self.keep_X else None, lam, torch.cat(stats, 1), torch.stack(statuses),
                               self.dfs(lam, M))

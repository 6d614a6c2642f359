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

Not there: localisation, more than 64 members, additive inflation, correlated observation errors, observation operators
that are not pointwise in the decoded frame.  No reference counterpart: the reference never assimilates.
"""
import collections

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

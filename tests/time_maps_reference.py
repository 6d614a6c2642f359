"""References of the per-pixel time maps (include/lns.h "time maps"; lns_op_time_maps, lns_rollout_eval_maps), in torch, on
whatever device the inputs live on.

`statement64`: the statement of include/lns.h as a sequential float64 loop over the selected steps, every operation a torch
op of its own (nothing can be fused), the running maximum in fp32 with torch.fmax (which skips a NaN as fmaxf does).  The
kernels are held to it bit for bit.  `Accumulator` is the same loop with its state exposed, so that a horizon can be fed in
chunks.  `direct64`: the seven maps from independent float64 reductions (mean / unbiased var / covariance / mse / amax over the
time axis) of the same denormalised fp32 fields.  `own32`: the same from torch's fp32 reductions -- the `own` of the project's
rule max(2e-7, 3 x own).

Layouts: y_hat, y [B, T, C, H, W] normalised fp32 -> [B, C, 7, H, W] in the order of NAMES.  `norm`: the keyword arguments of
lns_amd.engine.eval_spec."""
import torch

from ensemble_score_reference import denorm

NAMES = ("mean_P", "mean_Q", "var_P", "var_Q", "cov", "mse", "max_err")
FAMILIES = ("unit", "tiny", "huge", "offset", "drift")


def selected(T, map_from=0, map_every=1, t0=0):
    """The selected steps of the horizon that fall into the chunk [t0, t0 + T): t >= map_from, (t - map_from) % map_every == 0."""
    return [t for t in range(t0, t0 + T) if t >= map_from and (t - map_from) % map_every == 0]


def family(name, shape, g, device="cpu"):
    """-> (forecast, truth) [B, T, C, H, W] fp32: truth x ~ N(0, 1) scaled / shifted / drifting in time, forecast = truth plus
    noise of 0.3 of its standard deviation."""
    x = torch.randn(shape, device=device, generator=g)
    t = torch.arange(shape[1], device=device, dtype=torch.float32).view(1, -1, 1, 1, 1)
    q = {"unit": x, "tiny": 1e-12 * x, "huge": 1e12 * x, "offset": 1e3 + 1e-2 * x, "drift": x + 0.05 * t}[name].float()
    return (q + 0.3 * q.std() * torch.randn(shape, device=device, generator=g)).float(), q


class Accumulator:
    """The state of the statement for fields [B, C, H, W]: six float64 sums and the fp32 running maximum, from zero."""

    def __init__(self, K):
        self.K = K.double()                                   # D_c of the truth's first frame, fp32 values
        z = torch.zeros_like(self.K)
        self.Sa, self.Sb, self.Saa, self.Sbb, self.Sab, self.See = (z.clone() for _ in range(6))
        self.mx = torch.zeros_like(K, dtype=torch.float32)
        self.n = 0

    def add(self, P, Q):
        """One selected step: P, Q [B, C, H, W] denormalised fp32."""
        P, Q = P.double(), Q.double()
        a, b, e = P - self.K, Q - self.K, P - Q
        aa, bb, ab, ee = a * a, b * b, a * b, e * e
        self.Sa = self.Sa + a
        self.Sb = self.Sb + b
        self.Saa = self.Saa + aa
        self.Sbb = self.Sbb + bb
        self.Sab = self.Sab + ab
        self.See = self.See + ee
        self.mx = torch.fmax(self.mx, e.abs().float())
        self.n += 1

    def finish(self):
        """-> [B, C, 7, H, W] fp32"""
        assert self.n >= 1
        N = torch.full_like(self.K, float(self.n))
        d = torch.full_like(self.K, float(max(self.n - 1, 1)))
        zero = torch.zeros_like(self.K)

        def second(Sxy, Sx, Sy):
            t = Sx * Sy
            k = t / N
            return (Sxy - k) / d
        vP, vQ = second(self.Saa, self.Sa, self.Sa), second(self.Sbb, self.Sb, self.Sb)
        vP, vQ = torch.where(vP > 0, vP, zero), torch.where(vQ > 0, vQ, zero)
        maps = [self.K + self.Sa / N, self.K + self.Sb / N, vP, vQ, second(self.Sab, self.Sa, self.Sb), self.See / N]
        return torch.stack([m.float() for m in maps] + [self.mx], 2)


def statement64(y_hat, y, map_from=0, map_every=1, chunks=None, **norm):
    """The statement.  chunks: a list of chunk lengths summing to T -- the horizon is then walked chunk by chunk, each deriving
    its selected steps from (t0, T) alone, as the chunked streaming calls do."""
    T = y.shape[1]
    P, Q = denorm(y_hat, norm), denorm(y, norm)               # fp32 [B, T, C, H, W]
    acc = Accumulator(Q[:, 0])
    t0 = 0
    for n in ([T] if chunks is None else chunks):
        for t in selected(n, map_from, map_every, t0):
            acc.add(P[:, t], Q[:, t])
        t0 += n
    assert t0 == T
    return acc.finish()


def _pick(y_hat, y, map_from, map_every, norm, dtype):
    idx = selected(y.shape[1], map_from, map_every)
    return denorm(y_hat, norm)[:, idx].to(dtype), denorm(y, norm)[:, idx].to(dtype)


def _direct(P, Q):
    n = P.shape[1]
    mP, mQ = P.mean(1), Q.mean(1)
    if n > 1:
        vP, vQ = P.var(1, unbiased=True), Q.var(1, unbiased=True)
        cov = ((P - mP.unsqueeze(1)) * (Q - mQ.unsqueeze(1))).sum(1) / (n - 1)
    else:
        vP, vQ, cov = torch.zeros_like(mP), torch.zeros_like(mP), torch.zeros_like(mP)
    e = P - Q
    return torch.stack([mP, mQ, vP, vQ, cov, (e * e).mean(1), e.abs().amax(1)], 2)


def direct64(y_hat, y, map_from=0, map_every=1, **norm):
    """The maps from float64 reductions of the denormalised fp32 fields -> float64 [B, C, 7, H, W]."""
    return _direct(*_pick(y_hat, y, map_from, map_every, norm, torch.float64))


def own32(y_hat, y, map_from=0, map_every=1, **norm):
    """The same from torch's fp32 reductions -> fp32 [B, C, 7, H, W]."""
    return _direct(*_pick(y_hat, y, map_from, map_every, norm, torch.float32))

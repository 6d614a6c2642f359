"""References of the ensemble validation (include/lns.h "ensemble validation"; lns_op_ensemble_score,
lns_rollout_latent_ensemble_eval), in torch, on whatever device the inputs live on.

`statement32`: the statement of include/lns.h as explicit elementwise fp32 ops, one kernel per op, so nothing is fused;
divisors and the denormalisation's constants are device tensors (torch turns a division by a host scalar into a
multiplication by its reciprocal, which is not the correctly rounded quotient).  The kernel is held to it bit for bit.
`plane_scores32`: the reduction order and the finish kernel of the statement on such per-pixel values, again bit for bit.
`scores64`: every output in float64 from the same fp32 inputs (the denormalisation's constants rounded to fp32 first, as
the lns_eval_spec holds them).  `scores32_torch`: the same quantities from torch's own fp32 reductions -- the `own` of the
project's rule max(2e-7, 3 x own).

Layouts: frames [n, B, M, C, H, W] (a frame buffer), y [B, n, C, H, W]; per-pixel results [n, B, C, H, W]; scores
[B, n, C, 4] = rel_l2, rmse, spread, crps; seq [B, C, 4]; rank [B, n, C, M + 1].  `norm`: the keyword arguments of
lns_amd.engine.eval_spec."""
import torch


def _norm(C, mean=0.0, std=1.0, eps=1e-8, zero_wall_channels=(), clamp_channels=(), clamp=(0.0, 1.0 + 1e-8)):
    """-> (mean [C], std [C], zero flags [C], clamp flags [C], lo, hi, eps) as Python lists / floats."""
    def per_c(v):
        return [float(v)] * C if isinstance(v, (int, float)) else [float(e) for e in v]
    return (per_c(mean), per_c(std), [c in tuple(zero_wall_channels) for c in range(C)],
            [c in tuple(clamp_channels) for c in range(C)], float(clamp[0]), float(clamp[1]), float(eps))


def denorm(x, norm, dtype=torch.float32):
    """D_c of include/lns.h on x [..., C, H, W]: x * std_c + mean_c (two rounded ops), 0 on the wall rows / columns of the
    flagged channels, fmin(fmax(., lo), hi) on the clamped ones.  The constants are rounded to fp32 first."""
    C, H, W = x.shape[-3:]
    mean, std, zero, clampc, lo, hi, _ = _norm(C, **norm)
    dev = x.device

    def const(v):
        return torch.tensor(v, dtype=torch.float32, device=dev).to(dtype)
    p = x.to(dtype) * const(std).view(C, 1, 1)
    v = p + const(mean).view(C, 1, 1)
    if any(zero):
        border = torch.zeros((H, W), dtype=torch.bool, device=dev)
        border[0, :] = border[-1, :] = True
        border[:, 0] = border[:, -1] = True
        mask = torch.tensor(zero, device=dev).view(C, 1, 1) & border
        v = torch.where(mask, torch.zeros_like(v), v)
    if any(clampc):
        cl = torch.fmin(torch.fmax(v, const(lo)), const(hi))
        v = torch.where(torch.tensor(clampc, device=dev).view(C, 1, 1).expand(C, H, W), cl, v)
    return v


def pixels32(v, q):
    """The per-pixel part of the statement on denormalised fp32 values: v [M, ...], q [...] -> mu, var, crps (fp32), rank (int64)."""
    M = v.shape[0]
    fm = torch.full_like(q, float(M))
    fm1 = torch.full_like(q, float(M - 1))
    fpairs = torch.full_like(q, float(M * (M - 1)))
    s = v[0].clone()
    for m in range(1, M):
        s = s + v[m]
    mu = s / fm
    sd = torch.zeros_like(q)
    qq = torch.zeros_like(q)
    a = torch.zeros_like(q)
    rank = torch.zeros(q.shape, dtype=torch.int64, device=q.device)
    for m in range(M):
        d = v[m] - mu
        p = d * d
        sd = sd + d
        qq = qq + p
        t = v[m] - q
        a = a + t.abs()
        rank = rank + (v[m] < q)
    c = sd * sd
    k = c / fm
    nn = qq - k
    var = nn / fm1
    w = torch.zeros_like(q)
    for m in range(M - 1):
        for n in range(m + 1, M):
            t = v[m] - v[n]
            w = w + t.abs()
    t0 = a / fm
    t1 = w / fpairs
    return mu, var, t0 - t1, rank


def statement32(frames, y, **norm):
    """-> mu, var, crps (fp32) and rank (int64), each [n, B, C, H, W]."""
    v = denorm(frames, norm).permute(2, 0, 1, 3, 4, 5).contiguous()          # [M, n, B, C, H, W]
    q = denorm(y, norm).permute(1, 0, 2, 3, 4).contiguous()                  # [n, B, C, H, W]
    return pixels32(v, q)


def plane_sums32(x):
    """x [n, B, C, H, W] fp32 -> [B, n, C]: the statement's order.  Thread t of 256 adds pixels t, t + 256, ... in ascending
    order starting from 0; the wave sum and the four-wave sum are a balanced binary tree over the 256 thread sums in thread
    order (every level adds neighbours; fp32 addition is commutative)."""
    n, B, C = x.shape[:3]
    flat = x.reshape(n, B, C, -1)
    HW = flat.shape[-1]
    pad = (-HW) % 256
    if pad:
        flat = torch.cat([flat, torch.zeros((n, B, C, pad), dtype=x.dtype, device=x.device)], -1)
    rows = flat.view(n, B, C, -1, 256)
    acc = torch.zeros((n, B, C, 256), dtype=x.dtype, device=x.device)
    for r in range(rows.shape[3]):
        # a thread without a pixel in the last pass adds nothing (x + 0 = x, also for -0: the sum started from +0)
        acc = acc + rows[:, :, :, r]
    while acc.shape[-1] > 1:
        acc = acc[..., 0::2] + acc[..., 1::2]
    return acc[..., 0].permute(1, 0, 2).contiguous()


def _div32(a, b):
    """The correctly rounded fp32 quotient: the float64 quotient of fp32 operands rounds to it (53 >= 2 * 24 + 2 bits)."""
    return (a.double() / b.double()).float()


def _sqrt32(a):
    return a.double().sqrt().float()


def plane_scores32(mu, var, crps, q, eps):
    """Per-pixel mu, var, crps and the denormalised truth q, each [n, B, C, H, W] fp32 -> (scores [B, n, C, 4], seq [B, C, 4])
    with the bits of the statement: plane sums in its order, then its finish kernel, the steps summed in ascending order."""
    e = mu - q
    SE, G, V, CR = plane_sums32(e * e), plane_sums32(q * q), plane_sums32(var), plane_sums32(crps)
    n, HW = mu.shape[0], mu.shape[-2] * mu.shape[-1]
    fhw = torch.full_like(SE, float(HW))
    epsv = torch.full_like(SE, eps)
    scores = torch.stack([_sqrt32(_div32(SE, torch.where(G < epsv, epsv, G))), _sqrt32(_div32(SE, fhw)), _sqrt32(_div32(V, fhw)),
                          _div32(CR, fhw)], -1)
    tot = [torch.zeros_like(SE[:, 0]) for _ in range(4)]
    for t in range(n):
        tot = [a + b[:, t] for a, b in zip(tot, (SE, G, V, CR))]
    fall = torch.full_like(tot[0], float(n * HW))
    epsv = torch.full_like(tot[0], eps)
    seq = torch.stack([_sqrt32(_div32(tot[0], torch.where(tot[1] < epsv, epsv, tot[1]))), _sqrt32(_div32(tot[0], fall)),
                       _sqrt32(_div32(tot[2], fall)), _div32(tot[3], fall)], -1)
    return scores, seq, dict(SE=SE, G=G, V=V, CR=CR)


def rank_histogram(rank, M):
    """rank [n, B, C, H, W] (any integer or float dtype holding 0 .. M) -> counts [B, n, C, M + 1] int64."""
    n, B, C = rank.shape[:3]
    flat = rank.reshape(n, B, C, -1).permute(1, 0, 2, 3).reshape(B * n * C, -1).long()
    planes = torch.arange(B * n * C, device=rank.device).view(-1, 1) * (M + 1)
    return torch.bincount((flat + planes).reshape(-1), minlength=B * n * C * (M + 1)).view(B, n, C, M + 1)


def pair_sum_sorted(v):
    """sum_{m < n} |v_m - v_n| over dim 0 as sum_k (2 k - M + 1) v_(k) of the sorted values."""
    M = v.shape[0]
    coef = (2 * torch.arange(M, device=v.device, dtype=v.dtype) - (M - 1)).view((M,) + (1,) * (v.dim() - 1))
    return (coef * v.sort(dim=0).values).sum(0)


def finish(SE, G, V, CR, HW, eps):
    """Plane sums [B, n, C] -> (scores [B, n, C, 4], seq [B, C, 4]) in the sums' dtype."""
    n = SE.shape[1]
    e = torch.full_like(G, eps)
    scores = torch.stack([(SE / torch.where(G < e, e, G)).sqrt(), (SE / HW).sqrt(), (V / HW).sqrt(), CR / HW], -1)
    sSE, sG, sV, sCR = SE.sum(1), G.sum(1), V.sum(1), CR.sum(1)
    e = torch.full_like(sG, eps)
    seq = torch.stack([(sSE / torch.where(sG < e, e, sG)).sqrt(), (sSE / (n * HW)).sqrt(), (sV / (n * HW)).sqrt(), sCR / (n * HW)], -1)
    return scores, seq


def _plane(t):
    """[n, B, C, H, W] -> per-plane sums [B, n, C]"""
    return t.sum((-2, -1)).permute(1, 0, 2)


def scores64(frames, y, **norm):
    """Every output in float64 -> dict(mu, var, crps [n,B,C,H,W]; SE, G, V, CR [B,n,C]; scores; seq; rank [B,n,C,M+1])."""
    M = frames.shape[2]
    H, W = frames.shape[-2:]
    v = denorm(frames, norm, torch.float64).permute(2, 0, 1, 3, 4, 5)
    q = denorm(y, norm, torch.float64).permute(1, 0, 2, 3, 4)
    mu = v.mean(0)
    var = v.var(dim=0, unbiased=True)
    crps = (v - q).abs().mean(0) - pair_sum_sorted(v) / (M * (M - 1))
    rank = (v < q).sum(0)
    SE, G, V, CR = _plane((mu - q) ** 2), _plane(q * q), _plane(var), _plane(crps)
    scores, seq = finish(SE, G, V, CR, H * W, _norm(frames.shape[3], **norm)[6])
    return dict(mu=mu, var=var, crps=crps, SE=SE, G=G, V=V, CR=CR, scores=scores, seq=seq, rank=rank_histogram(rank, M))


def scores32_torch(frames, y, **norm):
    """The same quantities from torch's fp32 mean / var / abs().sum() (the pair term as one [M, M, ...] difference) ->
    dict(SE, G, V, CR, scores, seq) in fp32."""
    M = frames.shape[2]
    H, W = frames.shape[-2:]
    v = denorm(frames, norm).permute(2, 0, 1, 3, 4, 5)
    q = denorm(y, norm).permute(1, 0, 2, 3, 4)
    mu = v.mean(0)
    var = v.var(dim=0, unbiased=True)
    crps = (v - q).abs().sum(0) / M - (v[:, None] - v[None]).abs().sum((0, 1)) / (2 * M * (M - 1))
    SE, G, V, CR = _plane((mu - q) ** 2), _plane(q * q), _plane(var), _plane(crps)
    scores, seq = finish(SE, G, V, CR, H * W, _norm(frames.shape[3], **norm)[6])
    return dict(SE=SE, G=G, V=V, CR=CR, scores=scores, seq=seq)

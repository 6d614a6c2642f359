"""References of the ensemble quantiles (include/lns.h "ensemble quantiles"; lns_op_ensemble_quantiles,
lns_rollout_latent_ensemble_quantiles), in torch / numpy, on whatever device the inputs live on.

`statement32`: the statement of include/lns.h as explicit elementwise fp32 ops, one kernel per op, so nothing is fused; the
sort goes through the integer key of the statement (held in int64 and compared as the unsigned 32-bit number it is), the
interpolation weight and the member count are device tensors.  The kernel is held to it bit for bit (NaN as NaN).
`quantiles64`: numpy.quantile(..., method="linear") in float64 on the same fp32 inputs (the denormalisation's constants rounded
to fp32 first, as the lns_eval_spec holds them), the exceedance count taken in float64.
`own32`: torch.quantile in fp32 on the device and a `>` mean -- the `own` of the project's rule max(2e-7, 3 x own).

Layouts: frames [n, B, M, C, H, W] (a frame buffer); quantiles [B, n, n_q, C, H, W]; prob [B, n, n_thr, C, H, W].
`norm`: the keyword arguments of lns_amd.engine.eval_spec, or none for the values as they are."""
import math

import numpy as np
import torch

from ensemble_score_reference import denorm


def positions(quantiles, M):
    """[(lo, frac)]: h = p (M - 1) in double, lo = floor(h), frac = (float)(h - lo); lo = M - 1 forces frac = 0."""
    out = []
    for p in quantiles:
        h = float(p) * (M - 1)
        lo = int(math.floor(h))
        frac = float(np.float32(h - lo))
        out.append((M - 1, 0.0) if lo >= M - 1 else (lo, frac))
    return out


def thresholds_per_channel(thresholds, C):
    """each threshold a scalar (every channel) or C values -> [n_thr][C] floats, rounded to fp32 as the spec holds them"""
    rows = []
    for t in thresholds:
        row = [float(t)] * C if isinstance(t, (int, float)) else [float(v) for v in t]
        assert len(row) == C
        rows.append([float(np.float32(v)) for v in row])
    return rows


def to_key(v):
    """fp32 -> key(x) = bits ^ (sign ? 0xFFFFFFFF : 0x80000000) as a non-negative int64"""
    bits = v.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    sign = bits >= 0x80000000
    return bits ^ torch.where(sign, torch.full_like(bits, 0xFFFFFFFF), torch.full_like(bits, 0x80000000))


def from_key(key):
    """the inverse of to_key: a key with the top bit set came from a non-negative value"""
    pos = key >= 0x80000000
    bits = key ^ torch.where(pos, torch.full_like(key, 0x80000000), torch.full_like(key, 0xFFFFFFFF))
    bits = torch.where(bits >= 0x80000000, bits - 0x100000000, bits)
    return bits.to(torch.int32).view(torch.float32)


def sort_members(v, descending=False):
    """v [M, ...] fp32 -> sorted along dim 0 by the integer key"""
    return from_key(to_key(v).sort(dim=0, descending=descending).values)


def interpolate32(vs, pos):
    """vs [M, ...] sorted -> [n_q, ...]: frac == 0: v_(lo); otherwise d = v_(lo+1) - v_(lo), t = frac * d, v_(lo) + t"""
    rows = []
    for lo, frac in pos:
        if frac == 0.0:
            rows.append(vs[lo].clone())
            continue
        d = vs[lo + 1] - vs[lo]
        t = torch.full_like(d, frac) * d
        rows.append(vs[lo] + t)
    return torch.stack(rows, 0)


def exceed32(v, thr_rows, ge=False):
    """v [M, ..., C, H, W], thr_rows [n_thr][C] -> [n_thr, ..., C, H, W]: (float)#{m : v_m > thr} / (float)M"""
    M, C = v.shape[0], v.shape[-3]
    fm = torch.full(v.shape[1:], float(M), dtype=torch.float32, device=v.device)
    rows = []
    for row in thr_rows:
        th = torch.tensor(row, dtype=torch.float32, device=v.device).view(C, 1, 1)
        cnt = ((v >= th) if ge else (v > th)).sum(0).to(torch.float32)
        rows.append(cnt / fm)
    return torch.stack(rows, 0)


def members(frames, norm):
    """frames [n, B, M, C, H, W] -> the denormalised members [M, B, n, C, H, W]"""
    v = denorm(frames, norm) if norm else frames
    return v.permute(2, 1, 0, 3, 4, 5).contiguous()


def statement32(frames, quantiles=(), thresholds=(), **norm):
    """-> (quantiles [B, n, n_q, C, H, W] or None, prob [B, n, n_thr, C, H, W] or None), fp32"""
    M, C = frames.shape[2], frames.shape[3]
    v = members(frames, norm)
    quant = prob = None
    if len(quantiles):
        quant = interpolate32(sort_members(v), positions(quantiles, M)).permute(1, 2, 0, 3, 4, 5).contiguous()
    if len(thresholds):
        prob = exceed32(v, thresholds_per_channel(thresholds, C)).permute(1, 2, 0, 3, 4, 5).contiguous()
    return quant, prob


def quantiles64(frames, quantiles=(), thresholds=(), **norm):
    """numpy.quantile(method="linear") and the exceedance count in float64 -> (quantiles, prob) as float64 tensors on the CPU"""
    M, C = frames.shape[2], frames.shape[3]
    v = (denorm(frames, norm, torch.float64) if norm else frames.double()).permute(2, 1, 0, 3, 4, 5).cpu().numpy()
    quant = prob = None
    if len(quantiles):
        q = np.quantile(v, np.asarray([float(p) for p in quantiles], dtype=np.float64), axis=0, method="linear")
        quant = torch.from_numpy(np.ascontiguousarray(np.transpose(q, (1, 2, 0, 3, 4, 5))))
    if len(thresholds):
        rows = []
        for row in thresholds_per_channel(thresholds, C):
            th = np.asarray(row, dtype=np.float64).reshape(C, 1, 1)
            rows.append((v > th).sum(0).astype(np.float64) / float(M))
        prob = torch.from_numpy(np.ascontiguousarray(np.transpose(np.stack(rows, 0), (1, 2, 0, 3, 4, 5))))
    return quant, prob


def own32(frames, quantiles=(), thresholds=(), **norm):
    """torch.quantile in fp32 and a `>` mean on the inputs' device -> (quantiles, prob) in fp32"""
    M, C = frames.shape[2], frames.shape[3]
    v = members(frames, norm)
    quant = prob = None
    if len(quantiles):
        q = torch.quantile(v, torch.tensor([float(p) for p in quantiles], dtype=torch.float32, device=v.device), dim=0,
                           interpolation="linear")
        quant = q.permute(1, 2, 0, 3, 4, 5).contiguous()
    if len(thresholds):
        rows = [(v > torch.tensor(row, dtype=torch.float32, device=v.device).view(C, 1, 1)).float().mean(0)
                for row in thresholds_per_channel(thresholds, C)]
        prob = torch.stack(rows, 0).permute(1, 2, 0, 3, 4, 5).contiguous()
    return quant, prob

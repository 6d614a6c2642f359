"""The exceedance contingency tables of include/lns.h ("ensemble exceedance") stated on their own, for the tests: numpy
comparisons and counting with `np.add.at`, and the verification scores in float64 written from their definitions, per pixel
-- not from the binned formulas of `lns_amd.metrics`, which this file does not import.

Layouts: frames [n, B, M, C, H, W] (a frame buffer's), y [B, n, C, H, W]; table int32 [B, n, K, C, 2, M + 1]."""
import numpy as np


def thresholds_per_channel(thresholds, C):
    """thresholds (each a scalar for every channel or a per-channel sequence) -> float32 [K, C]"""
    rows = []
    for t in thresholds:
        row = [float(t)] * C if isinstance(t, (int, float)) else [float(v) for v in t]
        assert len(row) == C
        rows.append(row)
    return np.asarray(rows, dtype=np.float32).reshape(len(rows), C)


def denorm(x, norm, clamp=True):
    """D_c of include/lns.h on float32 x [..., C, H, W]: x * std_c, then + mean_c (each rounded to fp32 on its own), then 0 on
    the wall rows / columns of `zero_wall_channels`, then fmin(fmax(., lo), hi) on `clamp_channels`.  norm None: x itself."""
    x = np.asarray(x, dtype=np.float32)
    if norm is None:
        return x
    C, H, W = x.shape[-3:]

    def per_c(v):
        v = [float(v)] * C if isinstance(v, (int, float)) else [float(e) for e in v]
        assert len(v) == C
        return np.asarray(v, dtype=np.float32).reshape(C, 1, 1)
    p = (x * per_c(norm.get("std", 1.0))).astype(np.float32)
    v = (p + per_c(norm.get("mean", 0.0))).astype(np.float32)
    for c in norm.get("zero_wall_channels", ()):
        v[..., c, 0, :] = 0.0
        v[..., c, H - 1, :] = 0.0
        v[..., c, :, 0] = 0.0
        v[..., c, :, W - 1] = 0.0
    if clamp:
        lo, hi = (np.float32(b) for b in norm.get("clamp", (0.0, 1.0 + 1e-8)))
        for c in norm.get("clamp_channels", ()):
            v[..., c, :, :] = np.fmin(np.fmax(v[..., c, :, :], lo), hi)
    return v


def events(frames, y, thresholds, norm=None):
    """-> (x bool [K, n, B, M, C, H, W]: member m above threshold k, o bool [K, B, n, C, H, W]: the truth above it).  A NaN
    compares false."""
    frames, y = np.asarray(frames, dtype=np.float32), np.asarray(y, dtype=np.float32)
    C = frames.shape[3]
    thr = thresholds_per_channel(thresholds, C)
    v, q = denorm(frames, norm), denorm(y, norm)
    with np.errstate(invalid="ignore"):
        x = np.stack([v > thr[k].reshape(C, 1, 1) for k in range(len(thr))])
        o = np.stack([q > thr[k].reshape(C, 1, 1) for k in range(len(thr))])
    return x, o


def counts(frames, y, thresholds, norm=None):
    """-> (n int64 [K, B, n, C, H, W]: members above the threshold, o int64 [K, B, n, C, H, W]: 1 where the truth is); what
    `events` says, summed over the members threshold by threshold"""
    frames, y = np.asarray(frames, dtype=np.float32), np.asarray(y, dtype=np.float32)
    C = frames.shape[3]
    thr = thresholds_per_channel(thresholds, C)
    v, q = denorm(frames, norm), denorm(y, norm)
    with np.errstate(invalid="ignore"):
        nn = np.stack([(v > thr[k].reshape(C, 1, 1)).sum(2, dtype=np.int64).transpose(1, 0, 2, 3, 4) for k in range(len(thr))])
        o = np.stack([(q > thr[k].reshape(C, 1, 1)).astype(np.int64) for k in range(len(thr))])
    return nn, o


def table(frames, y, thresholds, norm=None):
    """The table of the statement: table[b][i][k][c][o][n] = number of pixels of plane (b, i, c) with that (o, n)."""
    n_steps, B, M, C, H, W = np.asarray(frames).shape
    nn, o = counts(frames, y, thresholds, norm)
    K = nn.shape[0]
    out = np.zeros((B, n_steps, K, C, 2, M + 1), dtype=np.int32)
    k, b, i, c = np.meshgrid(np.arange(K), np.arange(B), np.arange(n_steps), np.arange(C), indexing="ij")
    shape = nn.shape
    idx = tuple(np.broadcast_to(a.reshape(a.shape + (1, 1)), shape).reshape(-1) for a in (b, i, k, c))
    np.add.at(out, idx + (o.reshape(-1), nn.reshape(-1)), 1)
    return out


# ---- the scores, from their definitions, per pixel (float64) ---------------------------------------------------------------
def brier(n, o, M):
    """mean over the pixels of (n / M - o)^2"""
    n, o = np.asarray(n, dtype=np.float64).reshape(-1), np.asarray(o, dtype=np.float64).reshape(-1)
    return float(np.mean((n / M - o) ** 2))


def brier_fair(x, o):
    """The fair Brier score from the member indicators x [M, pixels] and the truth's o [pixels]: per pixel
    (1 / M) sum_m (x_m - o)^2 - (1 / (2 M (M - 1))) sum_{m, m'} (x_m - x_m')^2, the second term absent for M = 1."""
    x, o = np.asarray(x, dtype=np.float64), np.asarray(o, dtype=np.float64)
    M = x.shape[0]
    first = ((x - o[None]) ** 2).sum(0) / M
    second = np.zeros_like(first)
    if M > 1:
        for m in range(M):
            for mm in range(M):
                second += (x[m] - x[mm]) ** 2
        second /= 2.0 * M * (M - 1)
    return float(np.mean(first - second))


def brier_terms(n, o, M):
    """(reliability, resolution, uncertainty, base rate) by looping over the forecast values that occur"""
    n, o = np.asarray(n).reshape(-1), np.asarray(o, dtype=np.float64).reshape(-1)
    N = n.size
    base = o.mean()
    rel = res = 0.0
    for j in range(M + 1):
        sel = n == j
        if not sel.any():
            continue
        obar = o[sel].mean()
        rel += sel.sum() * (j / M - obar) ** 2
        res += sel.sum() * (obar - base) ** 2
    return rel / N, res / N, float(base * (1.0 - base)), float(base)


def mann_whitney(n, o):
    """P(n_event > n_other) + P(equal) / 2 over all (event pixel, other pixel) pairs, counted one by one; NaN without a pair"""
    n, o = np.asarray(n).reshape(-1), np.asarray(o).reshape(-1)
    ev, ot = n[o == 1], n[o == 0]
    if ev.size == 0 or ot.size == 0:
        return float("nan")
    s = 0.0
    for a in ev:
        for b in ot:
            s += 1.0 if a > b else (0.5 if a == b else 0.0)
    return s / (ev.size * ot.size)


def iou(forecast, truth):
    """|A and B| / |A or B| of two boolean masks; NaN when both are empty"""
    forecast, truth = np.asarray(forecast, dtype=bool), np.asarray(truth, dtype=bool)
    union = (forecast | truth).sum()
    return float((forecast & truth).sum() / union) if union else float("nan")


# ---- the inputs of the tests ------------------------------------------------------------------------------------------------
SCALAR = dict(mean=0.25, std=1.5)                     # maps the quantised family's 0, 1/2 and -1/2 onto the thresholds 1/4, 1 and -1/2
THRESHOLDS = (0.25, -0.5, "per_channel", 0.0, 1.0, -1.0, 0.5, "per_channel_2")


def per_channel_norm(C):
    """walls on channel 0 and the clamp on the last channel (both on the only channel of C = 1); about a third of the clamped
    channel's values sit at either bound, where the thresholds 0 and 1 meet them"""
    return dict(mean=[0.25 * c for c in range(C - 1)] + [0.5], std=[1.0 + 0.5 * c for c in range(C - 1)] + [0.5],
                zero_wall_channels=(0,), clamp_channels=(C - 1,), clamp=(0.0, 1.0))


def thresholds_for(C, n_thr=8):
    rows = [[0.5 - 0.25 * c for c in range(C)] if t == "per_channel" else [0.75 * c - 0.25 for c in range(C)] if t == "per_channel_2"
            else t for t in THRESHOLDS]
    return tuple(rows[:n_thr])


def family_fields(shape_frames, seed, shift=0):
    """numpy frames [n, B, M, C, H, W] and truth y [B, n, C, H, W] whose pixels cycle through the five input families --
    gaussian; quantised to 1/4 (ties with the thresholds, so the strict > decides); zeros; gaussian with one +inf or -inf
    member (and an infinite truth); gaussian with one NaN member (and, on every other such pixel, a NaN truth)."""
    n, B, M, C, H, W = shape_frames
    rng = np.random.default_rng(seed)
    gx = rng.standard_normal(shape_frames, dtype=np.float32)
    gy = rng.standard_normal((n, B, 1, C, H, W), dtype=np.float32)
    x, y = gx * np.float32(1.5) + np.float32(0.25), gy * np.float32(1.5) + np.float32(0.25)
    idx = np.arange(n * B * C * H * W).reshape(n, B, 1, C, H, W)
    fam = (idx + shift) % 5
    member = np.arange(M).reshape(1, 1, M, 1, 1, 1)
    xq, yq = np.round(gx * np.float32(4.0)) / np.float32(4.0), np.round(gy * np.float32(4.0)) / np.float32(4.0)
    x = np.where(fam == 1, xq, x)
    y = np.where(fam == 1, yq, y)
    x = np.where(fam == 2, np.float32(0.0), x)
    y = np.where(fam == 2, np.float32(0.0), y)
    hit = member == (idx // 5) % M
    inf = np.where((idx // 5) % 2 == 0, np.float32(np.inf), np.float32(-np.inf))
    x = np.where((fam == 3) & hit, inf, x)
    y = np.where(fam == 3, -inf, y)
    x = np.where((fam == 4) & hit, np.float32(np.nan), x)
    y = np.where((fam == 4) & ((idx // 5) % 2 == 1), np.float32(np.nan), y)
    return np.ascontiguousarray(x.astype(np.float32)), np.ascontiguousarray(y[:, :, 0].transpose(1, 0, 2, 3, 4).astype(np.float32))

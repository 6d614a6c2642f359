"""TEST INFRASTRUCTURE ONLY -- GroupNorm from the tile statistics of the producing convolution (lns_op_conv_gn): the case grid,
its deterministic inputs, and float64 statements of everything the kernels compute.  numpy and float64 torch; nothing outside
the repository is read.

What is stated here, all in float64:
  tile_pixels      which pixels of the plane partial `t` covers (the tile geometry lns_op_conv_gn reports, or `expected_geom`)
  partials64       per-(sample, tile, channel) (mean, M2 = sum (v - mean)^2, n) over a tile's valid pixels
  merge64          partials -> the group (scale, shift) table: scale = rstd gamma [premul], shift = beta - mean rstd gamma, the
                   statistics being those of y * premul (Chan et al.: M2 = sum_t M2_t + n_t (mean_t - mean)^2); optionally with
                   one of MISTAKES applied (tests/test_conv_gn_stats_cpu.py: the grid's inputs must tell each from the truth)
  groupnorm64      the normalisation itself, straight from the tensor
  fold64           normalisation -> activation -> consumer convolution (gpu_checks.conv_case_fp64)
Every comparison on the GPU takes the stored output y of the producer, read back and promoted, as the tensor: the producer's
own rounding, which the convolution tests gate, cancels, and only the statistics are judged.

Bounds of the per-tile partials (`partial_bounds`), from the summation tree of the epilogue (convb_epilogue, `stats` block):
four threads per channel take 32 pixels each.  Exact tiles: four stride-4 chains of 8 additions, (s0 + s1) + (s2 + s3), an
exact scaling by 1/32, then two pairwise merges mean = 0.5 (a + b) -- 7 + 2 + 2 = 11 roundings on the longest path of a value to
the mean.  Ragged tiles: the same chains masked, two quad additions and one division by the count -- 7 + 2 + 2 + 1 = 12.  With
the standard bound |fl(sum) - sum| <= k u sum |v_i| and sum |v_i| / n <= max |v|:
    |mean - mean64| <= t := MEAN_ROUNDINGS u max|v|,    MEAN_ROUNDINGS = 16 >= 12,  u = 2^-24.
M2: each 32-pixel (or masked whole-tile) sum of squares is taken about a computed mean m' = m + d, |d| <= t, and
sum (v - m')^2 = M2 + n d^2; the pairwise merges add 16 (m'_0 - m'_1)^2, 16 (m'_2 - m'_3)^2 and 32 (m'_01 - m'_23)^2.  As a
function of the four perturbations this is M2 + L + Q with (Cauchy-Schwarz against 16 d01^2 + 16 d23^2 + 32 D^2 <= M2)
|L| <= 32 sqrt(M2) t <= 3 sqrt(n M2) t for n = 128 and Q <= 3 n t^2; the ragged form has the n d^2 term alone.  Rounding: a
term passes the subtraction, the square, 7 + 2 additions and two merges of two additions each, < 32 roundings of non-negative
quantities.  Hence
    |M2 - M2_64| <= 3 sqrt(n M2_64) t + 3 n t^2 + 32 u (M2_64 + n t^2).
"""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

KERNEL_TOL = 2e-6          # tests/test_gpu_parity.py
STAGE_TOL = 2e-5
U = 2.0 ** -24
MEAN_ROUNDINGS = 16
TILE = 128
MISTAKES = ("ragged_as_128", "drop_between", "unweighted_mean", "premul_mean_only")
KINDS = ("random", "big_mean", "tile_ramp", "const_group", "sample_scales", "gamma_zero")
MIXED = ("random", "big_mean", "tile_ramp", "const_group", "small")         # the B = 5 case: one kind per sample
CONST = 3.25
# producer forms: kernel size, forced tile variant of lns_op_conv2d, 2x-upsampling phase form, padding modes (y, x)
PRODUCERS = {
    "c3": dict(k=3, variant=11, up=False),       # f16x2 3x3, 64-cout tiles
    "c3h": dict(k=3, variant=13, up=False),      # f16x2 3x3, 32-cout tiles: half the threads take statistics
    "up": dict(k=3, variant=17, up=True),        # phase form of the upsampling conv: four partials per source tile
    "c1": dict(k=1, variant=7, up=False),        # streaming 1x1: flat 128-pixel tiles
}
# consumers of the fold: (variant2, ksize2, act_in2)
CONSUMERS = [(11, 3, 1), (13, 3, 0), (7, 1, 1)]


def _case(prod, H, W, C, groups, kind="random", feature=None, premul=False, B=2, Cin=None):
    """H, W: the plane the GroupNorm sees (an upsampling producer reads H/2 x W/2)."""
    if Cin is None:
        Cin = 64 if C == 512 else (C if kind == "mixed" else 32)
    name = "%s-%dx%d-C%dg%d-%s" % (prod, H, W, C, groups, kind)
    name += ("-" + feature if feature else "") + ("-premul" if premul else "") + ("-B%d" % B if B != 2 else "")
    return dict(name=name, prod=prod, H=H, W=W, Cin=Cin, Cout=C, groups=groups, kind=kind, feature=feature, premul=premul, B=B)


def _grid():
    g = []
    planes = [("c3", 16, 16), ("c3", 32, 32), ("c3", 7, 15), ("c3", 14, 30), ("c3", 28, 60), ("c3h", 16, 16), ("c3h", 7, 15),
              ("up", 16, 32), ("up", 32, 32), ("c1", 16, 16), ("c1", 7, 15), ("c1", 14, 30)]
    for p, H, W in planes:                                       # every producer form and plane
        g.append(_case(p, H, W, 64, 32))
        g.append(_case(p, H, W, 128, 1))
    for p, H, W in [("c3", 16, 16), ("c3", 7, 15), ("c1", 16, 16), ("c1", 7, 15)]:      # the foldable planes: the other two
        g.append(_case(p, H, W, 64, 1))
        g.append(_case(p, H, W, 128, 32))
    for p, H, W in [("c3", 16, 16), ("c3", 14, 30), ("c3h", 7, 15), ("c1", 14, 30)]:    # cg = 25, ragged cout tile
        g.append(_case(p, H, W, 100, 4))
    for H, W in [(16, 16), (7, 15)]:                             # the fold's channel limit
        g.append(_case("c1", H, W, 512, 1))
    for kind in KINDS[1:]:
        for p, H, W, C, G in [("c3", 16, 16, 64, 32), ("c3", 7, 15, 128, 1), ("c3", 28, 60, 64, 32), ("c1", 14, 30, 128, 1),
                              ("up", 16, 32, 64, 32), ("c3", 32, 32, 64, 1)]:
            g.append(_case(p, H, W, C, G, kind))
    for feature in ("res", "badd_gelu", "oct"):
        for p, H, W, C, G in [("c3", 16, 16, 64, 32), ("c3", 7, 15, 64, 1), ("c3", 14, 30, 64, 32), ("c1", 16, 16, 64, 32)]:
            g.append(_case(p, H, W, C, G, "random", feature))
    # premul (the conditional two-phase blocks: ragged planes; exact ones by the same rule): one group folds, several finalize
    for p, H, W, C, G in [("c3", 7, 15, 64, 1), ("c3", 7, 15, 128, 1), ("c1", 7, 15, 64, 1), ("c3", 7, 15, 64, 32),
                          ("c3", 14, 30, 64, 32), ("c1", 14, 30, 100, 4), ("c3", 16, 16, 64, 1), ("c3", 16, 16, 64, 32)]:
        g.append(_case(p, H, W, C, G, "random", None, True))
    g.append(_case("c3", 14, 30, 64, 1, "tile_ramp", None, True))
    g.append(_case("c3", 16, 16, 64, 32, "mixed", B=5))
    g.append(_case("c3", 7, 15, 64, 1, "mixed", B=5))
    g.append(_case("c1", 14, 30, 64, 32, "mixed", B=5))
    assert len({c["name"] for c in g}) == len(g)
    return g


GRID = _grid()
BY_NAME = {c["name"]: c for c in GRID}


def eps_of(case):
    return 1e-6 if case["groups"] == 32 else 1e-5           # the two GroupNorm flavours of the models


def sample_kind(case, b):
    return MIXED[b] if case["kind"] == "mixed" else case["kind"]


def ill_conditioned(case, b):
    """big_mean: y - mean is taken from a float32 mean rounded to 2^-24 |mean|, a few 1e-5 of the spread at a mean 200 spreads
    away, and y * scale carries scale's rounding times the same factor; nothing that keeps float32 statistics can undo it."""
    return sample_kind(case, b) == "big_mean"


def const_channels(case, b):
    """Channels of sample b that hold the single value CONST (kind const_group), as a slice, or None."""
    if sample_kind(case, b) != "const_group":
        return None
    cg = case["Cout"] // case["groups"]
    g = case["groups"] // 2
    return slice(g * cg, (g + 1) * cg)


def expected_rule(case):
    """(mode, foldable, tiles) the issue's statement of the planner rule gives for the case: mode 0 exact / 1 one ragged tile /
    2 ragged tiles; foldable: at most two partials, <= 512 channels, premul only with one group, channels per group a power of
    two <= 64 (or one group)."""
    geom = expected_geom(case)
    H, W, C, G = case["H"], case["W"], case["Cout"], case["groups"]
    tiles = geom[7]
    full = all(len(p) == TILE for p in tile_pixels(geom, H, W))
    mode = 1 if (tiles == 1 and H * W < TILE) else (0 if full else 2)
    cg = C // G
    fold = mode != 2 and tiles <= 2 and C <= 512 and (not case["premul"] or G == 1) and (G == 1 or (cg <= 64 and cg & (cg - 1) == 0))
    return mode, fold, tiles


def expected_geom(case):
    """The tiling the engine chooses for the producer, as lns_op_conv_gn reports it: (tiles_x, tiles_y, log2 tile width, flat,
    phase multiplier, mode, foldable, tiles); mode / foldable are left -1 here (expected_rule).  3x3: 128-pixel tiles BW x BH of
    least padded area over the (source) plane, ties in the order 32, 64, 16, 128, 8 of BW."""
    P = PRODUCERS[case["prod"]]
    H, W = case["H"], case["W"]
    if P["k"] == 1:
        tx = (H * W + TILE - 1) // TILE
        return (tx, 1, 7, 1, 1, -1, -1, tx)
    if P["up"]:
        H, W = H // 2, W // 2
    best = None
    for lb in (5, 6, 4, 7, 3):
        BW, BH = 1 << lb, TILE >> lb
        cost = -(-H // BH) * BH * (-(-W // BW) * BW)
        if best is None or cost < best[0]:
            best = (cost, lb)
    lb = best[1]
    BW, BH = 1 << lb, TILE >> lb
    tx, ty, pm = -(-W // BW), -(-H // BH), 4 if P["up"] else 1
    return (tx, ty, lb, 0, pm, -1, -1, tx * ty * pm)


def tile_pixels(geom, H, W):
    """[flat pixel indices (row-major over the H x W plane) of partial t], valid pixels only."""
    tx, ty, lb, flat, pm = geom[:5]
    if flat:
        return [np.arange(TILE * t, min(TILE * (t + 1), H * W)) for t in range(tx)]
    BW, BH = 1 << lb, TILE >> lb
    out = []
    for j in range(ty):
        for i in range(tx):
            rows, cols = np.arange(j * BH, (j + 1) * BH), np.arange(i * BW, (i + 1) * BW)
            if pm == 1:
                rr, cc = rows[rows < H], cols[cols < W]
                out.append((rr[:, None] * W + cc[None, :]).ravel())
            else:                                   # source tile (j, i): partial 4 (j tx + i) + 2 py + px
                for py in (0, 1):
                    for px in (0, 1):
                        rr, cc = 2 * rows + py, 2 * cols + px
                        rr, cc = rr[rr < H], cc[cc < W]
                        out.append((rr[:, None] * W + cc[None, :]).ravel())
    return out


# ---- inputs ---------------------------------------------------------------------------------------------------------
def case_inputs(case):
    """Everything the producer and the GroupNorm take, float32, a pure function of the case:
    x [B,Cin,Hs,Ws], w, bias (or None), res, badd, act_out, oct, gamma, beta, premul (or None), pad, mode."""
    P = PRODUCERS[case["prod"]]
    r = np.random.default_rng(zlib.crc32(case["name"].encode()))
    B, Cin, C, H, W, k = case["B"], case["Cin"], case["Cout"], case["H"], case["W"], P["k"]
    Hs, Ws = (H // 2, W // 2) if P["up"] else (H, W)
    kinds = [sample_kind(case, b) for b in range(B)]
    cg, g = C // case["groups"], case["groups"] // 2
    x = r.standard_normal((B, Cin, Hs, Ws))
    w = r.standard_normal((C, Cin, k, k)) * 1.5 / np.sqrt(Cin * k * k)
    bias = 0.7 + 0.1 * r.standard_normal(C)
    identity = case["kind"] in ("tile_ramp", "mixed")          # y = x[co % Cin] + bias: y's properties are x's
    if identity:
        w[:] = 0.0
        w[np.arange(C), np.arange(C) % Cin, k // 2, k // 2] = 1.0
        bias[:] = 0.0
        ramp = 4.0 * np.arange(Hs)[:, None] / Hs + 2.0 * np.arange(Ws)[None, :] / Ws
        for b, kd in enumerate(kinds):
            if kd == "tile_ramp":
                x[b] = ramp[None] + 0.05 * x[b]
            elif kd == "big_mean":
                x[b] = 200.0 + x[b]
            elif kd == "small":
                x[b] = 1e-4 * (0.7 + 1.5 * x[b])
            else:
                x[b] = 0.7 + 1.5 * x[b]
                if kd == "const_group":
                    assert Cin == C
                    x[b, g * cg:(g + 1) * cg] = CONST
    elif case["kind"] == "big_mean":                           # spread 1, mean 200 spreads away
        w *= 1.0 / 1.5
        bias = 200.0 + 0.1 * r.standard_normal(C)
    elif case["kind"] == "const_group":
        w[g * cg:(g + 1) * cg] = 0.0
        bias[g * cg:(g + 1) * cg] = CONST
    elif case["kind"] == "sample_scales":
        bias = None
        x *= np.array([1e-4, 2e3] * B)[:B, None, None, None]
    gamma = 1.0 + 0.1 * r.standard_normal(C)
    beta = 0.1 * r.standard_normal(C)
    if case["kind"] == "gamma_zero":
        gamma[::3] = 0.0
    f32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)      # noqa: E731
    feat = case["feature"]
    circ = 1 if H * W % TILE == 0 else 0                        # periodic where the models are (exact planes)
    return dict(x=f32(x), w=f32(w), bias=f32(bias), res=f32(r.standard_normal((B, C, H, W))) if feat == "res" else None,
                badd=f32(r.standard_normal((B, C))) if feat == "badd_gelu" else None, act_out=2 if feat == "badd_gelu" else 0,
                oct=feat == "oct", gamma=f32(gamma), beta=f32(beta),
                premul=f32(1.0 + 0.5 * r.standard_normal((B, C))) if case["premul"] else None,
                pad=(k // 2,) * 4, mode=(circ, circ), up=(H, W) if P["up"] else None)


def consumer_weights(case, ksize2, cout2=64):
    r = np.random.default_rng(zlib.crc32((case["name"] + "/consumer%d" % ksize2).encode()))
    C = case["Cout"]
    w2 = (r.standard_normal((cout2, C, ksize2, ksize2)) / np.sqrt(C * ksize2 * ksize2)).astype(np.float32)
    return w2, (0.1 * r.standard_normal(cout2)).astype(np.float32)


def producer64(case, inp=None):
    """The producer's output evaluated in float64 and rounded to float32: what stands in for the stored y where there is no
    GPU (tests/test_conv_gn_stats_cpu.py)."""
    import gpu_checks as gc
    i = inp or case_inputs(case)
    y = gc.conv_case_fp64(i["x"], i["w"], i["bias"], 1, 1, i["pad"], i["mode"], i["up"], None, 0, i["badd"], i["act_out"], i["res"])
    return y.astype(np.float32)


# ---- float64 statements -----------------------------------------------------------------------------------------------
def partials64(y, tiles):
    """y [B,C,H,W] -> (mean [B,T,C], M2 [B,T,C], n [T]) over each tile's valid pixels."""
    B, C = y.shape[:2]
    yf = np.asarray(y, np.float64).reshape(B, C, -1)
    mean = np.stack([yf[:, :, idx].mean(-1) for idx in tiles], 1)
    m2 = np.stack([((yf[:, :, idx] - yf[:, :, idx].mean(-1, keepdims=True)) ** 2).sum(-1) for idx in tiles], 1)
    return mean, m2, np.array([len(idx) for idx in tiles], np.float64)


def partial_bounds(y, tiles):
    """(bound of |mean - mean64|, bound of |M2 - M2_64|, the latter without its term linear in t), each [B,T,C]: the module
    docstring's derivation.  The third is not asserted: the ratio to it is printed to show how much of the bound is used."""
    B, C = y.shape[:2]
    yf = np.asarray(y, np.float64).reshape(B, C, -1)
    _, m2, n = partials64(y, tiles)
    t = MEAN_ROUNDINGS * U * np.stack([np.abs(yf[:, :, idx]).max(-1) for idx in tiles], 1)
    nn = n[None, :, None]
    quad = 3.0 * nn * t * t + 32.0 * U * (m2 + nn * t * t)
    return t, 3.0 * np.sqrt(nn * m2) * t + quad, quad


def merge64(mean, m2, n, groups, eps, gamma, beta, premul=None, mistake=None):
    """Partials -> (scale, shift) [B,C] each, float64 (Chan et al. with weights n_t)."""
    assert mistake is None or mistake in MISTAKES
    B, T, C = mean.shape
    cg = C // groups
    p = np.ones((B, C)) if premul is None else np.asarray(premul, np.float64)
    n = np.asarray(n, np.float64)
    if mistake == "ragged_as_128":
        n = np.full_like(n, float(TILE))
    pm = (p[:, None, :] * mean).reshape(B, T, groups, cg)
    pq = ((np.ones_like(p) if mistake == "premul_mean_only" else p * p)[:, None, :] * m2).reshape(B, T, groups, cg)
    nt = n[None, :, None, None]
    N = cg * n.sum()
    if mistake == "unweighted_mean":
        gm = pm.mean((1, 3))
    else:
        gm = (nt * pm).sum((1, 3)) / N
    between = 0.0 if mistake == "drop_between" else nt * (pm - gm[:, None, :, None]) ** 2
    var = (pq + between).sum((1, 3)) / N
    rstd = np.repeat(1.0 / np.sqrt(var + eps), cg, 1)
    gm = np.repeat(gm, cg, 1)
    ga, be = np.asarray(gamma, np.float64)[None], np.asarray(beta, np.float64)[None]
    return rstd * ga * p, be - gm * rstd * ga


def groupnorm_torch(y, groups, eps, gamma, beta, premul, dtype):
    """F.group_norm(y * premul) in `dtype` on the CPU, returned as float64 [B,C,H,W]."""
    yt = torch.from_numpy(np.ascontiguousarray(y)).to(dtype)
    if premul is not None:
        yt = yt * torch.from_numpy(np.ascontiguousarray(premul)).to(dtype)[:, :, None, None]
    out = F.group_norm(yt, groups, torch.from_numpy(np.ascontiguousarray(gamma)).to(dtype),
                       torch.from_numpy(np.ascontiguousarray(beta)).to(dtype), eps)
    return out.double().numpy()


def groupnorm64(y, groups, eps, gamma, beta, premul=None):
    return groupnorm_torch(y, groups, eps, gamma, beta, premul, torch.float64)


def apply_table(y, scale, shift):
    """y * scale + shift in float64 (scale, shift [B,C] of any float type)."""
    return np.asarray(y, np.float64) * np.asarray(scale, np.float64)[:, :, None, None] + np.asarray(shift, np.float64)[:, :, None, None]


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).sum() / (b ** 2).sum()))


def table_errors(case, y, scale, shift, inp):
    """[(sample, rel-L2 error of y * scale + shift against the float64 normalisation, own, bound)].  The constant channels of
    a const_group sample are left out of the norm (a whole constant sample: no row): they are judged by `const_check`, because
    a (scale, shift) table cannot subtract before it multiplies -- 3.25 scale and mean rstd gamma = 3.25 / sqrt(eps) gamma are
    rounded separately and cancel to a few ulps of 3.25e3 gamma, against values of order 1 elsewhere.
    own: torch's float32 CPU F.group_norm against float64, where the sample is ill-conditioned by construction; else 0."""
    ref = groupnorm64(y, case["groups"], eps_of(case), inp["gamma"], inp["beta"], inp["premul"])
    got = apply_table(y, scale, shift)
    r32 = None
    rows = []
    for b in range(y.shape[0]):
        keep = np.ones(y.shape[1], bool)
        cs = const_channels(case, b)
        if cs is not None:
            keep[cs] = False
        if not keep.any():
            continue
        own = 0.0
        if ill_conditioned(case, b):
            if r32 is None:
                r32 = groupnorm_torch(y, case["groups"], eps_of(case), inp["gamma"], inp["beta"], inp["premul"], torch.float32)
            own = rel(r32[b][keep], ref[b][keep])
        rows.append((b, rel(got[b][keep], ref[b][keep]), own, max(KERNEL_TOL, 3.0 * own)))
    return rows


CONST_ROUNDINGS = 4


def const_check(case, y, scale, shift, inp):
    """[(sample, max |3.25 scale + shift - beta| over the constant channels, its bound)].  The partials of a constant tile are
    exact (sums of n equal values 3.25, n <= 2^13, and their quotient), so mean = 3.25, var = 0, rstd = R = 1 / sqrt(eps) in
    float32, and scale = fl(R gamma), shift = fl(beta - fl(fl(3.25 R) gamma)): CONST_ROUNDINGS = 4 roundings of quantities of
    size |3.25 scale|, each <= 2^-24 relative -- held to 4 ulps (2^-23 relative) of |3.25 scale|."""
    rows = []
    for b in range(y.shape[0]):
        cs = const_channels(case, b)
        if cs is None:
            continue
        assert (y[b, cs] == np.float32(CONST)).all(), "the producer did not store the constant exactly"
        s, t = np.asarray(scale[b, cs], np.float64), np.asarray(shift[b, cs], np.float64)
        err = np.abs(CONST * s + t - np.asarray(inp["beta"][cs], np.float64))
        bound = CONST_ROUNDINGS * 2.0 ** -23 * np.abs(CONST * s)
        rows.append((b, float(err.max()), float(bound[np.argmax(err - bound)]), bool((err <= bound).all())))
    return rows


def fold64(case, y, inp, w2, b2, ksize2, act_in2, norm=None):
    """float64: GroupNorm(y) -> act_in2 -> the consumer's stride-1 "same" convolution with the producer's padding modes."""
    import gpu_checks as gc
    if norm is None:
        norm = groupnorm64(y, case["groups"], eps_of(case), inp["gamma"], inp["beta"], inp["premul"])
    p = ksize2 // 2
    return gc.conv_case_fp64(norm, w2, b2, 1, 1, (p, p, p, p), inp["mode"], None, None, act_in2, None, 0, None)


def fold_bounds(case, y, inp, w2, b2, ksize2, act_in2):
    """(float64 reference y2, [bound per sample], [own per sample]).  KERNEL_TOL; ill-conditioned samples max(KERNEL_TOL, 3 x
    own), own = the same pipeline with torch's float32 F.group_norm in front; a const_group sample is widened by what
    `const_check` allows its constant channels: |delta| <= 4 ulps of |3.25 scale| per element there, times the largest slope of
    the activation (1.1 for Swish), pushed through the consumer with |w2| -- a rigorous bound on the output perturbation."""
    import gpu_checks as gc
    eps, G = eps_of(case), case["groups"]
    ref = fold64(case, y, inp, w2, b2, ksize2, act_in2)
    B = y.shape[0]
    own = [0.0] * B
    if any(ill_conditioned(case, b) for b in range(B)):
        r32 = fold64(case, y, inp, w2, b2, ksize2, act_in2, norm=groupnorm_torch(y, G, eps, inp["gamma"], inp["beta"], inp["premul"], torch.float32))
        own = [rel(r32[b], ref[b]) if ill_conditioned(case, b) else 0.0 for b in range(B)]
    bounds = [max(KERNEL_TOL, 3.0 * o) for o in own]
    if any(const_channels(case, b) is not None for b in range(B)):
        E = np.zeros(y.shape)
        R = 1.0 / np.sqrt(eps)
        for b in range(B):
            cs = const_channels(case, b)
            if cs is not None:
                E[b, cs] = (CONST_ROUNDINGS * 2.0 ** -23 * CONST * R * np.abs(np.asarray(inp["gamma"][cs], np.float64)))[:, None, None]
        p = ksize2 // 2
        d = gc.conv_case_fp64(1.1 * E, np.abs(w2), None, 1, 1, (p, p, p, p), inp["mode"], None, None, 0, None, 0, None)
        for b in range(B):
            if const_channels(case, b) is not None:
                bounds[b] += float(np.sqrt((d[b] ** 2).sum() / (ref[b] ** 2).sum()))
    return ref, bounds, own

"""TEST INFRASTRUCTURE ONLY -- FABlock2D with in_proj inside the sandwich (csrc/fa_fused.inc through lns_op_fa_fused): the case
grid, its deterministic inputs, the float64 statement of the operation, and a model of where the design's accuracy ends.
numpy on the CPU; the native library is not imported and nothing outside the repository is read.

The statement, in float64 on the float32 inputs:
    G = x * scale + shift                                  (the in_norm GroupNorm as a (scale, shift) table; identity without one)
    P[h * dh + d] = sum_c W[h * dh + d, c] G[c]            (in_proj, 1x1, no bias)
    Y = Kx[b, h] P Ky[b, h]^T                              (the sandwich, per plane)
    out = (Y - mean) / sqrt(var_biased + eps) per plane when instnorm, else Y
    amax[b] = max |G[b]|, G formed as the float32 fused multiply-add of the float32 inputs
`own` is the same statement evaluated in float32, against the float64 one.  Every error is taken PER PLANE, in two measures:
rel-L2, and max |diff| / max |ref| (one wrong element comparable to the plane's largest fails even in a 4096-pixel plane).
Without InstanceNorm both are checks of absolute scale.

`model` is the arithmetic csrc/fa_fused.inc and csrc/lns_kernels.h document, not a copy of the kernel: G, W, P, U = P Ky^T, Kx and
Ky are each the sum of two fp16 terms of the value times a power of two (f16x2_scale: the bound lands in 2^14 .. 2^15) -- G by
`bound`, W by the pack scale (largest entry below 16000), P by max |G| of the sample x the largest absolute row sum of W x
(1 + 1e-6), U by that x the largest absolute row sum of Ky, Kx and Ky by their maxima --, the lo x lo product of every
matrix product is dropped, everything else is float64.  A value a factor 2^-k below its bound keeps 22 - k bits once its low
term reaches fp16's subnormals (k > 8 or so), and `model` says what that costs a plane.

Bounds (tests/test_fa_fused_gpu.py): per plane and measure max(KERNEL_TOL, 3 x own); for the families where the design keeps
fewer bits (RELAXED: quiet_channel below 2^-8, plane_spread) max(KERNEL_TOL, 3 x own, 3 x model), the factor 3 over the model
covering the fp32 accumulation it leaves out.  tests/test_fa_fused_cpu.py holds `model` below a third of KERNEL_TOL for every
other case -- the statement that the chosen inputs are inside the full-accuracy domain.

What that check decided about the inputs (the case changes, never the bound):
  sample_scales  per-sample magnitudes 2e3 and 0.05 with the tight bound.  G is split at ONE scale per launch (`bound`, a layer
                 constant), only P and U follow the sample's own maximum: the model gives the quiet sample 2.5e-7 at 0.05,
                 1.0e-6 at 0.01 and 1.0e-4 at 1e-4 (a ratio of 2^-24 to the loud one: eleven bits are left).
  big_shift      |shift| = 50 |gamma| with shifts and W entries all positive.  With random signs some planes' offsets
                 sum_c W[p, c] shift[c] cancel to the size of the signal while G carries float32's rounding of a value of
                 50: 2e-6 .. 1e-5 on those planes in `model` and 2e-6 .. 5e-6 in `own` alike -- conditioning, not the kernel's.
  quiet_channel  the selecting W rows carry 0.25, a typical entry.
"""
import functools
import zlib

import numpy as np

KERNEL_TOL = 2e-6          # tests/test_gpu_parity.py
EPS = 1e-5
GAP = 192                  # floats between the samples of a strided x
# the kernels: fa_fused2_kernel<2> (form 0, shipped), fa_fused_kernel<2> (1), fa_fused_g_kernel<2,2,2> (2), <2,1,1>, <4,1,1>
KERNELS = {
    "b0": dict(H=64, W=64, Cin=64, form=0), "b1": dict(H=64, W=64, Cin=64, form=1), "b2": dict(H=64, W=64, Cin=64, form=2),
    "s64": dict(H=32, W=32, Cin=64, form=0), "s128": dict(H=32, W=32, Cin=128, form=0),
}
QUIET = (0, 4, 8, 12, 16)                                   # quiet_channel(2^-k)
KINDS = ("plain", "heavy_w", "zero_row", "heavy_k", "sample_scales", "big_shift", "eps_regime") + \
        tuple("quiet%d" % k for k in QUIET) + ("plane_spread",)
RELAXED = ("quiet12", "quiet16", "plane_spread")
NEEDS_SS = ("sample_scales", "big_shift") + tuple("quiet%d" % k for k in QUIET)
DIM_GPB = [(16, 1), (16, 0), (32, 1), (32, 2), (32, 0), (48, 1), (48, 3), (48, 0), (64, 1), (64, 2), (64, 4), (64, 0)]
HEADS_B = [(1, 3), (2, 1), (1, 8), (3, 1), (1, 9), (1, 1), (2, 3), (1, 3), (1, 1), (3, 3), (1, 8), (2, 1), (1, 9)]
QUIET_CH = 5
SAMPLE_SCALES = (2e3, 0.05)
MISTAKES = ("no_transpose", "swap_kx_ky", "next_head_kernels", "groups_permuted", "unbiased_var", "no_eps", "sample_stats",
            "p_times_2", "w_hi_only", "g_hi_only", "no_shift", "sample_reversed")


def make_case(kern, dh, heads, B, gpb=0, kind="plain", b_rev=0, instnorm=1, strided=False, ss_null=False, tight=False, tag=""):
    k = KERNELS[kern]
    name = "%s-dh%dh%dB%d-g%d-%s" % (kern, dh, heads, B, gpb, kind)
    name += ("-rev" if b_rev else "") + ("" if instnorm else "-raw") + ("-strided" if strided else "")
    name += ("-noss" if ss_null else "") + ("-tight" if tight else "") + tag
    return dict(name=name, kern=kern, H=k["H"], W=k["W"], Cin=k["Cin"], form=k["form"], dh=dh, heads=heads, B=B, gpb=gpb, kind=kind,
                b_rev=b_rev, instnorm=instnorm, strided=strided, ss_null=ss_null, tight=tight)


def _grid():
    g = []
    for k, kern in enumerate(KERNELS):
        for i, kind in enumerate(KINDS):
            dh, gpb = DIM_GPB[(i + 5 * k) % len(DIM_GPB)]
            heads, B = HEADS_B[(i + k) % len(HEADS_B)]
            if kind == "sample_scales" and B < 2:
                B = 3
            ss_null = (i + 2 * k + 1) % 3 == 0 and kind not in NEEDS_SS
            # sample_scales: the planner's formula is a layer constant, it knows no per-sample factor
            tight = kind == "sample_scales" or ((i + 3 * k) % 4 == 2 and not kind.startswith("quiet"))
            instnorm = 1 if kind == "eps_regime" else int((i + 2 * k) % 3 != 0)
            g.append(make_case(kern, dh, heads, B, gpb, kind, b_rev=(i + k) % 2, instnorm=instnorm, strided=(i + k) % 4 == 1,
                               ss_null=ss_null, tight=tight))
    g.append(make_case("b0", 64, 2, 9, 0, "plain", b_rev=1))                      # the largest case
    assert len({c["name"] for c in g}) == len(g)
    return g


GRID = _grid()
BY_NAME = {c["name"]: c for c in GRID}


def relaxed(case):
    return case["kind"] in RELAXED


def gpb_of(case):
    """Plane groups per block the launch uses: the planner's automatic rule keeps one group per block below 512 blocks."""
    groups = case["dh"] // 16
    if case["gpb"]:
        return case["gpb"]
    gpb = 4
    while gpb > 1 and (groups % gpb or case["B"] * case["heads"] * (groups // gpb) < 512):
        gpb -= 1
    return gpb


def zero_plane(case):
    return case["heads"] * case["dh"] - 3 if case["kind"] == "zero_row" else None


def quiet_planes(case):
    """The planes whose W row selects the quiet channel alone: one per 16-plane group."""
    if not case["kind"].startswith("quiet"):
        return []
    return [g * 16 + 3 for g in range(case["heads"] * case["dh"] // 16)]


def fma32(x, scale, shift):
    """float32 fused multiply-add of float32 arrays: the product is exact in float64, the sum rounds once there and once
    more to float32 (a double rounding that differs from the fused operation by at most one ulp, rarely)."""
    return (x.astype(np.float64) * scale.astype(np.float64) + shift.astype(np.float64)).astype(np.float32)


def case_inputs(case):
    """x [B, Cin, H, W], ss [B, Cin, 2] or None, bound, w [heads * dh, Cin], kx [B, heads, H, H], ky [B, heads, W, W] (float32)
    and amax [B] (the statement's max |G|)."""
    r = np.random.default_rng(zlib.crc32(case["name"].encode()))
    B, Cin, H, W, heads, dh, kind = case["B"], case["Cin"], case["H"], case["W"], case["heads"], case["dh"], case["kind"]
    planes = heads * dh
    x = r.standard_normal((B, Cin, H, W))
    gamma = r.uniform(0.5, 1.5, Cin) * r.choice([-1.0, 1.0], Cin)
    beta = r.uniform(-0.5, 0.5, Cin)
    if kind == "big_shift":                                  # |shift| at 50 times the scaled spread, all of one sign
        beta = 50.0 * np.abs(gamma)
    if kind.startswith("quiet"):
        f = 2.0 ** -int(kind[5:])
        gamma[QUIET_CH] *= f
        beta[QUIET_CH] *= f
    if case["ss_null"]:
        gamma, beta = np.ones(Cin), np.zeros(Cin)
        x = x.astype(np.float32)
        ss = None
        scale, shift = np.ones((B, Cin), np.float32), np.zeros((B, Cin), np.float32)
    else:                                                    # a GroupNorm (one group) of samples with their own mean and spread
        x = (x * 10.0 ** r.uniform(-0.5, 0.5, (B, 1, 1, 1)) + r.uniform(-2.0, 2.0, (B, 1, 1, 1))).astype(np.float32)
        x64 = x.astype(np.float64)
        mean, var = x64.mean(axis=(1, 2, 3)), x64.var(axis=(1, 2, 3))
        rstd = 1.0 / np.sqrt(var + 1e-5)
        scale = rstd[:, None] * gamma[None]
        shift = beta[None] - mean[:, None] * scale
        if kind == "sample_scales":
            m = np.array([SAMPLE_SCALES[b % 2] for b in range(B)])
            scale, shift = scale * m[:, None], shift * m[:, None]
            gamma, beta = gamma * m.max(), beta * m.max()
        scale, shift = scale.astype(np.float32), shift.astype(np.float32)
        ss = np.ascontiguousarray(np.stack([scale, shift], axis=-1))
    g32 = fma32(x, scale[:, :, None, None], shift[:, :, None, None])
    amax = np.abs(g32).reshape(B, -1).max(axis=1)
    # the planner's a-priori bound of a GroupNorm output, one group: max |gamma| sqrt(Cin H W) + max |beta|
    bound = np.float32(amax.max()) if case["tight"] else np.float32(np.abs(gamma).max() * np.sqrt(Cin * H * W) + np.abs(beta).max())
    assert amax.max() <= bound
    w = (r.standard_t(2.0, (planes, Cin)) if kind == "heavy_w" else r.standard_normal((planes, Cin))) / np.sqrt(Cin)
    if kind == "big_shift":
        w = np.abs(w)
    if kind == "plane_spread":
        w = w * 10.0 ** r.uniform(-2.0, 2.0, (planes, 1))
    if kind == "zero_row":
        w[zero_plane(case)] = 0.0
    for p in quiet_planes(case):
        w[p] = 0.0
        w[p, QUIET_CH] = 0.25
    draw = (lambda s: r.standard_t(2.0, s)) if kind == "heavy_k" else r.standard_normal
    kx, ky = draw((B, heads, H, H)) / np.sqrt(H), draw((B, heads, W, W)) / np.sqrt(W)
    inp = dict(x=x, ss=ss, scale=scale, shift=shift, bound=bound, amax=amax, w=w.astype(np.float32), kx=kx.astype(np.float32),
               ky=ky.astype(np.float32))
    if kind == "eps_regime":                                 # plane variances around eps: InstanceNorm no longer hides a scale
        v = statement64(dict(case, instnorm=0), inp).var(axis=(2, 3))
        f = (1e-5 / np.exp(np.log(v).mean())) ** 0.25
        inp["kx"], inp["ky"] = (inp["kx"] * np.float32(f)).astype(np.float32), (inp["ky"] * np.float32(f)).astype(np.float32)
    return inp


def _instnorm(y, eps, unbiased=False, per_sample=False):
    ax = (1, 2, 3) if per_sample else (2, 3)
    mean = y.mean(axis=ax, keepdims=True)
    var = y.var(axis=ax, keepdims=True, ddof=1 if unbiased else 0)
    with np.errstate(divide="ignore", invalid="ignore"):        # (an all-zero plane without eps: NaN, an infinite error)
        return (y - mean) / np.sqrt(var + y.dtype.type(eps))


def _sandwich(p, kx, ky, case):
    """Y = Kx P Ky^T per (sample, head, plane); p [B, planes, H, W]."""
    B, heads, dh, H, W = case["B"], case["heads"], case["dh"], case["H"], case["W"]
    y = kx[:, :, None] @ p.reshape(B, heads, dh, H, W) @ np.swapaxes(ky, -1, -2)[:, :, None]
    return y.reshape(B, heads * dh, H, W)


def _hi16(v, s):
    """The high fp16 term of v at the power-of-two scale s."""
    return (v * s).astype(np.float32).astype(np.float16).astype(np.float64) / s


def statement64(case, inp, mistake=None):
    """The float64 statement [B, planes, H, W], optionally with one of MISTAKES."""
    B, Cin, H, W, heads, dh = case["B"], case["Cin"], case["H"], case["W"], case["heads"], case["dh"]
    x, w = inp["x"].astype(np.float64), inp["w"].astype(np.float64)
    kx, ky = inp["kx"].astype(np.float64), inp["ky"].astype(np.float64)
    scale, shift = inp["scale"].astype(np.float64), inp["shift"].astype(np.float64)
    if mistake == "no_shift":
        shift = np.zeros_like(shift)
    g = x * scale[:, :, None, None] + shift[:, :, None, None]
    if mistake == "g_hi_only":
        g = _hi16(g, pow2_scale(inp["bound"]))
    if mistake == "w_hi_only":
        w = _hi16(w, pack_scale(inp["w"]))
    if mistake == "sample_reversed":
        g = g[::-1]
    p = (w[None] @ g.reshape(B, Cin, H * W)).reshape(B, heads * dh, H, W)
    if mistake == "p_times_2":
        p = 2.0 * p
    if mistake == "groups_permuted":
        p = np.roll(p.reshape(B, heads, dh // 16, 16, H, W), 1, axis=2).reshape(p.shape)
    if mistake == "next_head_kernels":
        kx, ky = np.roll(kx, -1, axis=1), np.roll(ky, -1, axis=1)
    if mistake == "swap_kx_ky":
        kx, ky = ky, kx
    if mistake == "no_transpose":
        ky = np.swapaxes(ky, -1, -2)
    y = _sandwich(p, kx, ky, case)
    if not case["instnorm"]:
        return y
    return _instnorm(y, 0.0 if mistake == "no_eps" else EPS, unbiased=mistake == "unbiased_var", per_sample=mistake == "sample_stats")


def statement32(case, inp):
    """The same statement in float32 throughout."""
    B, Cin, H, W, heads, dh = case["B"], case["Cin"], case["H"], case["W"], case["heads"], case["dh"]
    g = inp["x"] * inp["scale"][:, :, None, None] + inp["shift"][:, :, None, None]
    p = (inp["w"][None] @ g.reshape(B, Cin, H * W)).reshape(B, heads * dh, H, W)
    y = _sandwich(p, inp["kx"], inp["ky"], case)
    assert y.dtype == np.float32
    return _instnorm(y, EPS) if case["instnorm"] else y


def pow2_scale(bound):
    """f16x2_scale (csrc/lns_kernels.hip): the power of two S with S * bound in [2^14, 2^15), exponent clamped to -110 .. 120."""
    bound = float(np.float32(bound))
    e = (np.frexp(bound)[1] - 1) if bound > 0.0 else -127
    return 2.0 ** min(120, max(-110, 14 - e))


def pack_scale(w):
    """The scale of the in_proj weight image: the largest entry lands below 16000."""
    wmax = float(np.abs(w).max())
    return 2.0 ** np.floor(np.log2(16000.0 / (wmax if wmax > 0.0 else 1.0)))


def _split(v, s):
    """v (float64) as two fp16 terms of fl32(v * s), returned at v's own scale."""
    t = (v * s).astype(np.float32)
    hi = t.astype(np.float16)
    lo = (t - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64) / s, lo.astype(np.float64) / s


def _per(scales, shape):
    return np.asarray(scales, np.float64).reshape(shape)


def model64(case, inp):
    """The documented arithmetic of the fused kernels (module docstring), [B, planes, H, W] float64."""
    B, Cin, H, W, heads, dh = case["B"], case["Cin"], case["H"], case["W"], case["heads"], case["dh"]
    g32 = fma32(inp["x"], inp["scale"][:, :, None, None], inp["shift"][:, :, None, None])
    gh, gl = _split(g32.astype(np.float64).reshape(B, Cin, H * W), pow2_scale(inp["bound"]))
    wh, wl = _split(inp["w"].astype(np.float64), pack_scale(inp["w"]))
    p = wh[None] @ gh + wh[None] @ gl + wl[None] @ gh
    wrow = np.float32(np.float32(np.abs(inp["w"]).sum(axis=1).max()) * np.float32(1.0 + 1e-6))
    bp = (inp["amax"].astype(np.float32) * wrow).astype(np.float32)                        # [B]
    ph, pl = _split(p.reshape(B, heads, dh, H, W), _per([pow2_scale(v) for v in bp], (B, 1, 1, 1, 1)))
    kx, ky = inp["kx"].astype(np.float64), inp["ky"].astype(np.float64)
    kxh, kxl = _split(kx, _per([pow2_scale(v) for v in np.abs(inp["kx"]).reshape(B * heads, -1).max(axis=1)], (B, heads, 1, 1)))
    kyh, kyl = _split(ky, _per([pow2_scale(v) for v in np.abs(inp["ky"]).reshape(B * heads, -1).max(axis=1)], (B, heads, 1, 1)))
    kyh, kyl = np.swapaxes(kyh, -1, -2)[:, :, None], np.swapaxes(kyl, -1, -2)[:, :, None]
    u = ph @ kyh + ph @ kyl + pl @ kyh
    br = np.abs(inp["ky"]).sum(axis=-1, dtype=np.float32).max(axis=-1)                      # [B, heads]
    bu = (bp[:, None] * br).astype(np.float32)
    uh, ul = _split(u, _per([pow2_scale(v) for v in bu.reshape(-1)], (B, heads, 1, 1, 1)))
    kxh, kxl = kxh[:, :, None], kxl[:, :, None]
    y = (kxh @ uh + kxh @ ul + kxl @ uh).reshape(B, heads * dh, H, W)
    return _instnorm(y, EPS) if case["instnorm"] else y


def plane_errors(out, ref):
    """(rel-L2, max |diff| / max |ref|) per plane, [B, planes] each; a plane whose reference is all zero: 0 if `out` is too,
    else inf; a plane of `out` with a non-finite element: inf."""
    bad = ~np.isfinite(out).all(axis=(2, 3))
    d = np.nan_to_num(out.astype(np.float64) - ref, nan=0.0, posinf=0.0, neginf=0.0)
    n2, m = np.sqrt((ref * ref).sum(axis=(2, 3))), np.abs(ref).max(axis=(2, 3))
    e2, em = np.sqrt((d * d).sum(axis=(2, 3))), np.abs(d).max(axis=(2, 3))
    with np.errstate(divide="ignore", invalid="ignore"):
        zero = np.where(em > 0, np.inf, 0.0)
        return np.where(bad, np.inf, np.where(m > 0, e2 / n2, zero)), np.where(bad, np.inf, np.where(m > 0, em / m, zero))


@functools.lru_cache(maxsize=None)
def reference(name):
    """Everything the tests of a case share, computed once: inputs, the float64 statement, per-plane (rel-L2, rel-max) errors
    of `own` and `model`, and the per-plane bounds in both measures."""
    case = BY_NAME[name]
    inp = case_inputs(case)
    ref = statement64(case, inp)
    own = plane_errors(statement32(case, inp), ref)
    model = plane_errors(model64(case, inp), ref)
    rounded = plane_errors(ref.astype(np.float32), ref)
    bounds = tuple(np.maximum(KERNEL_TOL, 3.0 * np.maximum(o, m if relaxed(case) else 0.0)) for o, m in zip(own, model))
    for a in (ref, inp["x"], inp["w"], inp["kx"], inp["ky"]):
        a.setflags(write=False)
    return dict(case=case, inp=inp, ref=ref, own=own, model=model, rounded=rounded, bounds=bounds)


# ---- a whole FABlock2D in float64 (the plan's block against the statement) -------------------------------------------------
def _erf(a):
    import torch
    return torch.special.erf(torch.from_numpy(np.ascontiguousarray(a))).numpy()


def _gelu64(a):
    return 0.5 * a * (1.0 + _erf(a / np.sqrt(2.0)))


def _layernorm64(a, g, b, eps=1e-5):
    m, v = a.mean(axis=-1, keepdims=True), a.var(axis=-1, keepdims=True)
    return (a - m) / np.sqrt(v + eps) * g + b


def _rotary64(t, inv_freq):
    """Rotary embedding at positions linspace(0, 1, n) / min_freq (1 / 64); t [b, h, n, d].  The ANGLES are float32, formed as
    torch.linspace and the float32 products of the module form them (they are part of the operation's definition: rounding
    an angle of up to 64 rad moves its cosine by 4e-6); cosine, sine and everything after them are float64."""
    n = t.shape[2]
    i = np.arange(n, dtype=np.float32)
    step = np.float32(1.0 / (n - 1)) if n > 1 else np.float32(0.0)
    pos = np.where(i < n // 2, step * i, np.float32(1.0) - step * (np.float32(n - 1) - i)).astype(np.float32)
    f = ((pos * np.float32(64.0))[:, None] * inv_freq.astype(np.float32)[None, :]).astype(np.float32).astype(np.float64)
    f = np.concatenate([f, f], axis=-1)
    d = t.shape[-1]
    rot = np.concatenate([-t[..., d // 2:], t[..., :d // 2]], axis=-1)
    return t * np.cos(f) + rot * np.sin(f)


def fa_block64(sd, pfx, x, heads):
    """FABlock2D (in_norm -> in_proj | to_in -> axis pooling -> reducers -> rotary low-rank kernels; sandwich -> InstanceNorm
    -> to_out; + x) in float64 from the float32 state dict `sd` and the float32 input x [B, C, H, W].  Returns the block's
    output and the operands of the fused kernels: the (scale, shift) table [B, C, 2], W, Kx, Ky and the sandwich's output."""
    g = lambda k: sd[pfx + k].astype(np.float64)
    lin = lambda a, w, b=None: a @ w.T + (0.0 if b is None else b)
    conv1 = lambda w, a: np.einsum("oc,bchw->bohw", w.reshape(w.shape[0], -1), a)
    B, C, H, W = x.shape
    x = x.astype(np.float64)
    mean, var = x.mean(axis=(1, 2, 3)), x.var(axis=(1, 2, 3))
    scale = (1.0 / np.sqrt(var + 1e-5))[:, None] * g(".in_norm.weight")[None]
    shift = g(".in_norm.bias")[None] - mean[:, None] * scale
    u = x * scale[:, :, None, None] + shift[:, :, None, None]
    for k in (".in_proj.weight", ".to_in.0.weight", ".to_out.1.weight", ".to_out.3.weight"):
        assert sd[pfx + k].shape[2:] == (1, 1), k

    def reducer(p, a):                                       # a [b, c, n, m] -> [b, n, out]: mean over m
        t = lin(a.transpose(0, 2, 3, 1), g(p + ".to_in.weight")).mean(axis=2)
        t = _layernorm64(t, g(p + ".out_ffn.0.weight"), g(p + ".out_ffn.0.bias"))
        return lin(_gelu64(lin(t, g(p + ".out_ffn.1.weight"))), g(p + ".out_ffn.3.weight"), g(p + ".out_ffn.3.bias"))

    def kernel(p, a):                                        # a [b, n, c] -> [b, heads, n, n]
        qk = lin(a, g(p + ".to_qk.weight"))
        half = qk.shape[-1] // 2
        sp = lambda t: t.reshape(B, t.shape[1], heads, half // heads).transpose(0, 2, 1, 3)
        q, k = (_rotary64(sp(t), sd[pfx + p + ".pos_emb.inv_freq"]) for t in (qk[..., :half], qk[..., half:]))
        return q @ np.swapaxes(k, -1, -2)

    t = conv1(g(".to_in.0.weight"), u)
    kx = kernel(".low_rank_kernel_x", reducer(".to_x.0", t))
    ky = kernel(".low_rank_kernel_y", reducer(".to_y.1", t.transpose(0, 1, 3, 2)))
    w = g(".in_proj.weight").reshape(-1, C)
    dh = w.shape[0] // heads
    case = dict(B=B, heads=heads, dh=dh, H=H, W=W)
    s = _instnorm(_sandwich(conv1(w, u), kx, ky, case), EPS)
    out = conv1(g(".to_out.3.weight"), _gelu64(conv1(g(".to_out.1.weight"), s))) + x
    return out, dict(ss=np.stack([scale, shift], axis=-1), w=w, kx=kx, ky=ky, sandwich=s, gamma=g(".in_norm.weight"), beta=g(".in_norm.bias"))

"""GPU (-m gpu): the ensemble quantiles (lns_op_ensemble_quantiles, lns_rollout_latent_ensemble_quantiles, include/lns.h;
Engine.ensemble_quantiles / rollout_latent_ensemble_quantiles, LatentDynamics.predict_quantiles, metrics.ensemble_quantiles).

References: tests/ensemble_quantile_reference.py.  The op is held BIT FOR BIT to `statement32` (the fp32 statement of
include/lns.h as explicit elementwise torch ops, the sort through the integer key); where the statement gives NaN the kernel
must give NaN, whatever the payload.  A result depends on its M inputs only, so there is nothing to tolerate.  Against float64
(`quantiles64`: numpy.quantile(method="linear") on the same fp32 inputs) the quantiles are held to the project's rule
max(2e-7, 3 x own), in max |diff| / max |ref| and in rel-L2 per output tensor, `own` being the float64 distance of
torch.quantile in fp32 on the device (`own32`); the probabilities must equal the float64 count over M, rounded to fp32, exactly.
The engine call is held bit for bit to the op on the member fields that `rollout_latent` at batch B * M with keep_steps produces."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import ensemble_quantile_reference as ref  # noqa: E402
from helpers import load_golden, case_args  # noqa: E402

pytestmark = pytest.mark.gpu

B, M, T = 2, 3, 7
NOISE = 0.05
KEEP_SETS = ([0], [6], [1, 4, 6], [0, 1, 2, 3, 4, 5, 6], [2, 3], [0, 2, 3, 4, 6])     # tests/test_rollout_ensemble_gpu.py's
DEFAULTS = dict(decode_group=1, decode_streams=3, overlap=1)
FLOOR = 2e-7
SENTINEL = -12345.0
PROBS = (0.0, 0.05, 0.25, 1.0 / 3.0, 0.5, 0.95, 1.0)
SCALAR = dict(mean=0.25, std=1.5)                     # maps the quantised family's 0 and -1/2 onto the thresholds 1/4 and -1/2
FAMILIES = ("gaussian", "quantised", "zeros", "inf", "nan")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _same(a, b):
    """equal bits, or NaN on both sides"""
    if a.shape != b.shape:
        return False
    a, b = a.contiguous(), b.contiguous()
    return bool(((a.view(torch.int32) == b.view(torch.int32)) | (torch.isnan(a) & torch.isnan(b))).all())


def per_channel_norm(C):
    """A per-channel spec with walls on channel 0 and the clamp on the last channel (both on the only channel of C = 1);
    the clamped channel's map puts about a third of the values at either bound, so members tie there."""
    return dict(mean=[0.25 * c for c in range(C - 1)] + [0.5], std=[1.0 + 0.5 * c for c in range(C - 1)] + [0.5],
                zero_wall_channels=(0,), clamp_channels=(C - 1,), clamp=(0.0, 1.0))


def thresholds_for(C):
    """three thresholds: two scalars the quantised family ties with, and a per-channel row"""
    return (0.25, -0.5, [0.5 - 0.25 * c for c in range(C)])


# ---- the op ------------------------------------------------------------------------------------------------------------
def _guarded(n, off):
    buf = torch.full((n + 12,), SENTINEL, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf, buf[4 + off:4 + off + n]


def _op(frames, probs, thresholds, norm, off_in=0, off_out=0, quant=True, prob=True, expect=0):
    """lns_op_ensemble_quantiles through ctypes; frames optionally one float off a 16-byte boundary; both outputs sit between
    sentinels that must survive, and an output that was not asked for stays untouched."""
    from lns_amd import _lib, engine
    L = _lib.lib()
    n, b, m, c, h, w = frames.shape
    probs = probs if quant else ()
    thresholds = thresholds if prob else ()
    qs = engine.quantile_spec(c, m, probs, thresholds)
    spec = engine.eval_spec(c, **norm) if norm else None
    buf = torch.empty(frames.numel() + 4, device="cuda")
    assert buf.data_ptr() % 16 == 0
    src = buf[off_in:off_in + frames.numel()]
    src.copy_(frames.reshape(-1))
    nq, nt = len(PROBS), 3
    outs = dict(quant=_guarded(b * n * nq * c * h * w, off_out), prob=_guarded(b * n * nt * c * h * w, off_out))
    want = dict(quant=quant, prob=prob)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.lns_op_ensemble_quantiles(src.data_ptr(), n, b, m, c, h, w, ctypes.byref(qs), ctypes.byref(spec) if spec is not None else None,
                                     outs["quant"][1].data_ptr() if quant else None, outs["prob"][1].data_ptr() if prob else None, stream)
    assert rc == expect, (rc, L.lns_create_error())
    torch.cuda.synchronize()
    for k, (full, view) in outs.items():
        lo = 4 + off_out
        assert bool((full[:lo] == SENTINEL).all()) and bool((full[lo + view.numel():] == SENTINEL).all()), k
        if not want[k] or rc != 0:
            assert bool((full == SENTINEL).all()), k
    return outs["quant"][1].view(b, n, nq, c, h, w), outs["prob"][1].view(b, n, nt, c, h, w)


def _family_frames(n, b, m, c, h, w, g, shift):
    """Member fields whose pixels cycle through the five input families (a result depends on its own pixel's members only):
    pixel (flat index over [n, b, c, h, w]) i has family (i + shift) % 5 --
    gaussian; quantised to 1/4 (ties between members and at the thresholds); a mix of +0 / -0; gaussian with one +inf or
    -inf member; gaussian with one NaN member."""
    shape = (n, b, m, c, h, w)
    x = torch.randn(shape, device="cuda", generator=g) * 1.5 + 0.25
    idx = torch.arange(n * b * c * h * w, device="cuda").view(n, b, 1, c, h, w)
    fam = ((idx + shift) % 5).expand(shape)
    member = torch.arange(m, device="cuda").view(1, 1, m, 1, 1, 1).expand(shape)
    quantised = (torch.randn(shape, device="cuda", generator=g) * 4.0).round() / 4.0
    signs = torch.where(torch.rand(shape, device="cuda", generator=g) < 0.5, -torch.zeros(shape, device="cuda"), torch.zeros(shape, device="cuda"))
    x = torch.where(fam == 1, quantised, x)
    x = torch.where(fam == 2, signs, x)
    hit = member == (idx // 5) % m                                         # the one member of the pixel that is replaced
    inf = torch.where((idx // 5) % 2 == 0, torch.full((), float("inf"), device="cuda"), torch.full((), float("-inf"), device="cuda"))
    x = torch.where((fam == 3) & hit, inf.expand(shape), x)
    x = torch.where((fam == 4) & hit, torch.full((), float("nan"), device="cuda").expand(shape), x)
    return x.contiguous()


SHAPES = [(b, n, c, hw) for b in (1, 3) for n in (1, 2) for c in (1, 3)
          for hw in ((1, 1), (3, 5), (16, 16), (257, 1), (17, 16), (61, 121))]


@pytest.mark.parametrize("m", [1, 2, 3, 33, 128])
def test_op_has_the_bits_of_the_statement(m):
    """B in {1, 3} x n in {1, 2} x C in {1, 3} x H x W in {1x1, 3x5, 16x16 (exactly one block), 257x1 and 17x16 (one block and a
    tail), 61x121}, without a norm and with the scalar spec, and 3x5 and 61x121 again with the per-channel spec (walls, clamp);
    seven probabilities and three thresholds; inputs and outputs aligned and one float off a 16-byte boundary; sentinels around
    both outputs, and an output that was not asked for stays untouched.  The pixels of every case cycle through the five input
    families (a result depends on its own pixel's members only); a case with fewer than 64 pixels is run with every shift of the
    cycle, so every family meets every shape.  The statement is evaluated once for all the cases of one M (it is elementwise:
    the pixels are concatenated per channel count)."""
    _need_gpu()
    g = torch.Generator(device="cuda")
    g.manual_seed(300 + m)
    cases = []
    for (b, n, c, (h, w)) in SHAPES:
        norms = (None, SCALAR) + ((per_channel_norm(c),) if (h, w) in ((3, 5), (61, 121)) else ())
        for norm in norms:
            for shift in (range(5) if b * n * c * h * w < 64 else (0,)):
                frames = _family_frames(n, b, m, c, h, w, g, shift)
                v = ref.members(frames, norm)                                  # [M, B, n, C, H, W]
                cases.append((frames, norm, v))
    pos = ref.positions(PROBS, m)
    want = []
    for frames, norm, v in cases:
        want.append(v.reshape(m, -1))
    flat = torch.cat(want, 1)
    fam_seen = (int(torch.isnan(flat).any()), int(torch.isinf(flat).any()), int(((flat == 0) & torch.signbit(flat)).any()))
    assert m == 1 or fam_seen == (1, 1, 1)
    quant_all = ref.interpolate32(ref.sort_members(flat), pos)                 # [n_q, pixels]
    at = 0
    for frames, norm, v in cases:
        n, b, _, c, h, w = frames.shape
        npx = v[0].numel()
        want_q = quant_all[:, at:at + npx].view((len(PROBS),) + tuple(v.shape[1:])).permute(1, 2, 0, 3, 4, 5).contiguous()
        at += npx
        thr = thresholds_for(c)
        want_p = ref.exceed32(v, ref.thresholds_per_channel(thr, c)).permute(1, 2, 0, 3, 4, 5).contiguous()
        for offs in ((0, 0), (1, 0), (0, 1)):
            quant, prob = _op(frames, PROBS, thr, norm, *offs)
            tag = (m, tuple(frames.shape), "none" if norm is None else ("scalar" if norm is SCALAR else "per_channel"), offs)
            assert _same(quant, want_q), tag
            assert _same(prob, want_p), tag
    # only one of the two outputs: the other stays untouched, the one asked for is the same
    frames, norm, v = cases[-1]
    thr = thresholds_for(frames.shape[3])
    both = _op(frames, PROBS, thr, norm)
    assert _same(_op(frames, PROBS, thr, norm, prob=False)[0], both[0])
    assert _same(_op(frames, PROBS, thr, norm, quant=False)[1], both[1])
    # the Python surfaces: Engine.ensemble_quantiles is the op; metrics.ensemble_quantiles is the statement
    from lns_amd import metrics
    res = _case("ns2d_mini")[2].ensemble_quantiles(frames, PROBS, thr, **(norm or {}))
    assert _same(res.quantiles, both[0]) and _same(res.prob, both[1]) and res.mean is None and res.var is None and res.z_last is None
    mq, mp = metrics.ensemble_quantiles(frames.permute(1, 2, 0, 3, 4, 5).contiguous(), PROBS, thr, **(norm or {}))
    assert _same(mq, both[0]) and _same(mp, both[1])


def test_op_refuses_member_counts_outside_1_128():
    _need_gpu()
    from lns_amd import _lib
    frames = torch.randn((1, 1, 129, 1, 2, 2), device="cuda")
    _op(frames, PROBS, thresholds_for(1), None, expect=_lib.LNS_EINVAL)
    assert "M in 1 .. 128" in _lib.lib().lns_create_error().decode()


def rule(ours, own, want, what, gate=True):
    """max(2e-7, 3 x own) against float64, in both measures -> the two ratios ours / bound."""
    want = want.to(ours.device)

    def errs(a):
        d = a.double() - want
        return float(d.abs().max() / want.abs().max()), float(d.norm() / want.norm())
    o, w = errs(ours), errs(own)
    ratios = [a / max(FLOOR, 3.0 * b) for a, b in zip(o, w)]
    print("%s: rel-max %.3e (own %.3e) rel-L2 %.3e (own %.3e) -> %.3f %.3f of the bound"
          % (what, o[0], w[0], o[1], w[1], ratios[0], ratios[1]))
    if gate:
        assert o[0] <= max(FLOOR, 3.0 * w[0]) and o[1] <= max(FLOOR, 3.0 * w[1]), (what, o, w)
    return ratios


def float64_families(m, g):
    """-> [(name, frames [n, B, M, C, H, W], thresholds)]: B = 2, n = 2, C = 3, 23 x 29 pixels (two blocks and a tail)"""
    base = torch.randn((2, 2, m, 3, 23, 29), device="cuda", generator=g)
    thr = (0.25, -0.5, [0.5, 0.25, 0.0])

    def scaled(s, o=0.0):
        return tuple([o + s * v for v in t] if isinstance(t, list) else o + s * t for t in thr)
    return [("normal", base, thr), ("1e-12", (1e-12 * base).contiguous(), scaled(1e-12)), ("1e12", (1e12 * base).contiguous(), scaled(1e12)),
            ("1e3 + 1e-2", (1e3 + 1e-2 * base).contiguous(), scaled(1e-2, 1e3))]


@pytest.mark.parametrize("m", [2, 7, 33, 128])
def test_op_quantiles_against_float64(m):
    """N(0,1), 1e-12 x, 1e12 x and 1e3 + 1e-2 x, without a norm (so the scale is the scale of what is interpolated): the
    quantiles under the rule max(2e-7, 3 x own) per output tensor, the probabilities equal to the float64 count over M rounded
    to fp32.  Every case prints its ratios; tools/ensemble_quantile_parity.py records the worst per family."""
    _need_gpu()
    g = torch.Generator(device="cuda")
    g.manual_seed(400 + m)
    for name, frames, thr in float64_families(m, g):
        quant, prob = _op(frames, PROBS, thr, None)
        q64, p64 = ref.quantiles64(frames, PROBS, thr)
        own, _ = ref.own32(frames, PROBS, thr)
        rule(quant, own, q64, "M=%d %s" % (m, name))
        assert torch.equal(prob.cpu(), p64.float()), (m, name)


# ---- the engine --------------------------------------------------------------------------------------------------------
_cases = {}


def _options(eng, **kw):
    for k, v in dict(DEFAULTS, **kw).items():
        if eng.options.get(k, DEFAULTS[k]) != v:
            eng.set_option(k, v)


def _case_norm(args):
    from lns_amd import metrics
    if args.family == "twophase_cond":
        return metrics.twophase_spec(0.1, 1.3, -0.2, 2.1)
    if args.family == "ns2d":
        return dict(mean=0.37, std=1.9)
    return dict(mean=[0.1 * c for c in range(args.in_channels)], std=[1.0 + 0.5 * c for c in range(args.in_channels)])


def _case(name):
    """(args, model, engine, x, z [B, M, c, h, w], param [B, M] or None, norm, thresholds, {}) -- built once per preset, as
    tests/test_rollout_ensemble_gpu.py does; never written afterwards."""
    if name not in _cases:
        import gpu_checks as gc
        from lns_amd import filler
        meta, _ = load_golden(name)
        args = case_args(meta)
        model, _ = gc.build_models(args, meta["weight_seed"])
        seed = meta["input_seed"]
        xd = torch.from_numpy(filler.normal("x", (B, args.in_channels, args.Ly, args.Lx), seed)).cuda()
        eng = model._engine(xd)
        _options(eng)
        z0 = model.x_to_z(xd)
        g = torch.Generator(device="cuda")
        g.manual_seed(seed)
        z = (z0[:, None] + torch.randn((B, M) + tuple(z0.shape[1:]), device="cuda", generator=g) * NOISE).contiguous()
        pd = torch.from_numpy(filler.uniform01("param", B * M, seed).astype(np.float32)).cuda().view(B, M) \
            if args.family == "twophase_cond" else None
        thr = (0.5, [0.1 * (c + 1) for c in range(args.in_channels)])
        _cases[name] = (args, model, eng, xd, z, pd, _case_norm(args), thr, {})
    return _cases[name]


def _want(name, steps, keep, with_norm=True):
    """What the op gives on the member fields rollout_latent at batch B * M with keep_steps produces, and
    rollout_latent_ensemble's mean / var / z_last; computed once per (steps, keep, norm) under the default options."""
    args, model, eng, xd, z, pd, norm, thr, refs = _case(name)
    key = (steps, tuple(keep), with_norm)
    if key not in refs:
        _options(eng)
        kept, _ = eng.rollout_latent(z.view((B * M,) + tuple(z.shape[2:])), steps, param=None if pd is None else pd.reshape(-1),
                                     keep_steps=keep)
        frames = kept.view((B, M) + tuple(kept.shape[1:])).permute(2, 0, 1, 3, 4, 5).contiguous()      # [n, B, M, C, Ly, Lx]
        op = eng.ensemble_quantiles(frames, PROBS, thr, **(norm if with_norm else {}))
        mean, var, z_last = eng.rollout_latent_ensemble(z, steps, param=pd, keep_steps=keep, return_last=True)
        torch.cuda.synchronize()
        refs[key] = (op, mean, var, z_last)
    return refs[key]


def _check(name, steps, keep, with_norm=True, outputs=True, twice=False):
    args, model, eng, xd, z, pd, norm, thr, _ = _case(name)
    opts = dict(eng.options)
    op, mean, var, z_last = _want(name, steps, keep, with_norm)
    _options(eng, **{k: opts.get(k, DEFAULTS[k]) for k in DEFAULTS})
    for _ in range(2 if twice else 1):
        got = eng.rollout_latent_ensemble_quantiles(z, steps, PROBS, thr, param=pd, keep_steps=keep, return_mean=outputs,
                                                    return_var=outputs, return_last=outputs, **(norm if with_norm else {}))
        torch.cuda.synchronize()
        tag = (name, keep, with_norm, eng.options)
        shape = (B, len(keep), len(PROBS), args.in_channels, args.Ly, args.Lx)
        assert tuple(got.quantiles.shape) == shape and tuple(got.prob.shape) == shape[:2] + (len(thr),) + shape[3:]
        assert _same(got.quantiles, op.quantiles) and _same(got.prob, op.prob), tag
        if outputs:
            assert _same(got.mean, mean) and _same(got.var, var) and _same(got.z_last, z_last), tag
        else:
            assert got.mean is None and got.var is None and got.z_last is None
    return got


GRID = [("ns2d_mini", dg, ds, 1) for dg in (1, 2, 3, 0) for ds in (1, 2, 3, 4)] + \
       [("ns2d_mini", dg, ds, 0) for dg in (1, 2, 3, 0) for ds in (1, 3)] + \
       [(c, dg, ds, 1) for c in ("twophase_cond", "sw_half_periodic") for dg in (1, 2) for ds in (1, 3)]


@pytest.mark.parametrize("case,dg,ds,ov", GRID)
def test_engine_quantiles_have_the_bits_of_the_op_on_the_member_rollouts(case, dg, ds, ov):
    """quantiles and prob of the call == lns_op_ensemble_quantiles on rollout_latent(z.view(B * M, ...), T, keep_steps) arranged
    as [n][B][M], bit for bit, for every scheduling option; mean, var and z_last are rollout_latent_ensemble's bits.
    twophase_cond runs with one parameter value per member and the per-channel spec (walls, clamp)."""
    _need_gpu()
    eng = _case(case)[2]
    try:
        for keep in KEEP_SETS:
            _want(case, T, keep)
            _options(eng, decode_group=dg, decode_streams=ds, overlap=ov)
            _check(case, T, keep)
    finally:
        _options(eng)


def test_quantiles_without_norm_alone_twice_and_in_the_diagnostic_modes():
    """Without a norm the values are normalised (the op without a norm); without mean / var / z_last (no reduction launch) the
    quantiles are the same; twice in a row on one workspace; more kept groups than ring groups and frame buffers; trace and
    timing modes (everything on the caller's stream); lns_check_finite covers the call."""
    _need_gpu()
    args, model, eng, xd, z, pd, norm, thr, _ = _case("ns2d_mini")
    keep = [1, 4, 6]
    try:
        _options(eng)
        _check("ns2d_mini", T, keep, with_norm=False)
        _check("ns2d_mini", T, keep, outputs=False, twice=True)
        _check("ns2d_mini", T, keep, twice=True)
        eng.check_finite(B * M, z.device)
        _options(eng, decode_group=1, decode_streams=3)
        steps = 2 * 5 + 4
        keep2 = [t for t in range(steps) if t not in (1, 5, 6)]
        _check("ns2d_mini", steps, keep2, twice=True)
        _options(eng, decode_group=2)
        eng.timing_enable(True)
        _check("ns2d_mini", T, keep)
        eng.timing_enable(False)
        eng.trace_enable(True)
        _check("ns2d_mini", T, keep)
        eng.trace_enable(False)
    finally:
        eng.timing_enable(False)
        eng.trace_enable(False)
        _options(eng)


def test_one_member_is_the_rollout_itself():
    """M = 1: every quantile equals rollout_latent(..., keep_steps), and every probability is 0 or 1."""
    _need_gpu()
    args, model, eng, xd, z, pd, norm, thr, _ = _case("ns2d_mini")
    _options(eng)
    keep = [1, 4, 6]
    z1 = z[:, :1].contiguous()
    want, _ = eng.rollout_latent(z1[:, 0].contiguous(), T, keep_steps=keep)
    got = eng.rollout_latent_ensemble_quantiles(z1, T, PROBS, thr, keep_steps=keep, return_mean=True)
    torch.cuda.synchronize()
    for k in range(len(PROBS)):
        assert _same(got.quantiles[:, :, k], want), k
    assert _same(got.mean, want)
    for k, row in enumerate(ref.thresholds_per_channel(thr, args.in_channels)):
        th = torch.tensor(row, device="cuda").view(-1, 1, 1)
        assert torch.equal(got.prob[:, :, k], (want > th).float())


def test_workspace_is_the_ensemble_rollouts_and_a_short_one_is_refused():
    _need_gpu()
    from lns_amd import _lib, engine
    args, model, eng, xd, z, pd, norm, thr, _ = _case("ns2d_mini")
    L, h = eng._L, eng._h
    keep = [1, 4, 6]
    op, mean_ref, var_ref, _ = _want("ns2d_mini", T, keep)
    _options(eng)
    n1 = ctypes.c_size_t(0)
    assert L.lns_rollout_ensemble_workspace_bytes(h, B, M, ctypes.byref(n1)) == 0
    C = args.in_channels
    quant = torch.full((B, 3, len(PROBS), C, args.Ly, args.Lx), SENTINEL, device="cuda")
    prob = torch.full((B, 3, len(thr), C, args.Ly, args.Lx), SENTINEL, device="cuda")
    mean = torch.full((B, 3, C, args.Ly, args.Lx), SENTINEL, device="cuda")
    var = torch.full_like(mean, SENTINEL)
    ws = torch.empty(n1.value, dtype=torch.uint8, device="cuda")
    qs = engine.quantile_spec(C, M, PROBS, thr)
    spec = engine.eval_spec(C, **norm)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run(nbytes):
        return L.lns_rollout_latent_ensemble_quantiles(h, z.data_ptr(), None, B, M, T, (ctypes.c_int * 3)(*keep), 3, ctypes.byref(qs),
                                                       ctypes.byref(spec), quant.data_ptr(), prob.data_ptr(), mean.data_ptr(),
                                                       var.data_ptr(), None, ws.data_ptr(), nbytes, stream)
    assert run(n1.value - 1) == _lib.LNS_ENOMEM and "ensemble workspace too small" in L.lns_last_error(h).decode()
    torch.cuda.synchronize()
    for t in (quant, prob, mean, var):
        assert bool((t == SENTINEL).all())                                   # nothing was enqueued
    assert run(n1.value) == 0                                                # exactly the ensemble rollout's workspace
    torch.cuda.synchronize()
    assert _same(quant, op.quantiles) and _same(prob, op.prob) and _same(mean, mean_ref) and _same(var, var_ref)


@pytest.mark.parametrize("case", ["ns2d_mini", "twophase_cond"])
def test_predict_quantiles_is_the_hand_written_composition(case):
    """x_to_z, randn with the same generator state, rollout_latent_ensemble_quantiles: equal bits; and for the same generator
    state its mean is predict_ensemble's."""
    _need_gpu()
    args, model, eng, xd, z, pd, norm, thr, _ = _case(case)
    _options(eng)
    members, keep = 4, [0, 3, 6]
    extra = (pd[:, 0].contiguous(),) if pd is not None else ()          # [B]: shared by a trajectory's members
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    got = model.predict_quantiles(xd, T, *extra, members, NOISE, quantiles=PROBS, thresholds=thr, generator=g, keep_steps=keep,
                                  return_mean=True, return_var=True, **norm)
    g.manual_seed(5)
    z0 = model.x_to_z(xd)
    eps = torch.randn((B, members) + tuple(z0.shape[1:]), device=z0.device, generator=g) * NOISE
    zz = z0[:, None] + eps
    zz[:, 0] = z0
    param = extra[0][:, None].expand(B, members).contiguous() if extra else None
    hand = eng.rollout_latent_ensemble_quantiles(zz, T, PROBS, thr, param=param, keep_steps=keep, **norm)
    g.manual_seed(5)
    mean, var = model.predict_ensemble(xd, T, *extra, members, NOISE, generator=g, keep_steps=keep)
    g.manual_seed(5)
    default = model.predict_quantiles(xd, T, *extra, members, NOISE, generator=g, keep_steps=keep)
    torch.cuda.synchronize()
    assert _same(got.quantiles, hand.quantiles) and _same(got.prob, hand.prob)
    assert _same(got.mean, mean) and _same(got.var, var)
    assert hand.mean is None and hand.var is None and hand.z_last is None
    assert default.prob is None and tuple(default.quantiles.shape) == (B, len(keep), 3, args.in_channels, args.Ly, args.Lx)
    assert bool((default.quantiles[:, :, 0] <= default.quantiles[:, :, 1]).all())
    assert bool((default.quantiles[:, :, 1] <= default.quantiles[:, :, 2]).all())

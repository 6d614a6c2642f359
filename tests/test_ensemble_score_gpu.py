"""GPU (-m gpu): the ensemble validation (lns_op_ensemble_score, lns_rollout_latent_ensemble_eval, include/lns.h;
Engine.ensemble_score / rollout_latent_ensemble_eval, LatentDynamics.validate_ensemble, metrics.spread_skill_ratio).

References: tests/ensemble_score_reference.py.  Per pixel the kernel is held BIT FOR BIT to `statement32` (the fp32
statement of include/lns.h as explicit elementwise torch ops) through the op's `pixel_out`, and its plane sums and
finished scores to `plane_scores32` (the statement's reduction order and finish kernel), also bit for bit: a result depends
on its inputs only and every order is fixed, so there is nothing to tolerate.  Against float64 of the same fp32 inputs
(`scores64`) the sums and scores are held to the project's rule max(2e-7, 3 x own), in max |diff| / max |ref| and in
rel-L2 per output tensor, `own` being the float64 distance of the same quantities from torch's own fp32 mean / var /
abs().sum() on the device (`scores32_torch`).  The engine call is held bit for bit to the op on the member fields that
`rollout_latent` at batch B * M produces."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import ensemble_score_reference as ref  # noqa: E402
from helpers import load_golden, case_args  # noqa: E402

pytestmark = pytest.mark.gpu

B, M, T = 2, 3, 7
NOISE = 0.05
KEEP_SETS = ([0], [6], [1, 4, 6], [0, 1, 2, 3, 4, 5, 6], [2, 3], [0, 2, 3, 4, 6])     # tests/test_rollout_ensemble_gpu.py's
DEFAULTS = dict(decode_group=1, decode_streams=3, overlap=1)
FLOOR = 2e-7
SENTINEL = -12345.0
ISENTINEL = -7777
SCALAR = dict(mean=0.37, std=1.9)
NAMES = ("rel_l2", "rmse", "spread", "crps")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def per_channel_norm(C):
    """A per-channel spec with walls on channel 0 and the clamp on the last channel (both on the only channel of C = 1);
    the clamped channel's map puts about a third of the values at either bound, so members tie there."""
    return dict(mean=[0.25 * c for c in range(C - 1)] + [0.5], std=[1.0 + 0.5 * c for c in range(C - 1)] + [0.5],
                zero_wall_channels=(0,), clamp_channels=(C - 1,), clamp=(0.0, 1.0))


# ---- the op ------------------------------------------------------------------------------------------------------------
def _guarded(n, off, dtype, fill):
    buf = torch.full((n + 12,), fill, dtype=dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf, buf[4 + off:4 + off + n]


def _op(frames, y, norm, off_f=0, off_y=0, off_out=0, rank=True, seq=True, pixel=True, expect=0):
    """lns_op_ensemble_score through ctypes; frames / y optionally one float off a 16-byte boundary; every output sits
    between sentinels that must survive (an output that was not asked for stays untouched)."""
    from lns_amd import _lib, engine
    L = _lib.lib()
    n, b, m, c, h, w = frames.shape
    spec = engine.eval_spec(c, **norm)
    ins = []
    for t, off in ((frames, off_f), (y, off_y)):
        buf = torch.empty(t.numel() + 4, device="cuda")
        assert buf.data_ptr() % 16 == 0
        view = buf[off:off + t.numel()]
        view.copy_(t.reshape(-1))
        ins.append(view)
    sizes = dict(scores=(b * n * c * 4, torch.float32, SENTINEL), seq=(b * c * 4, torch.float32, SENTINEL),
                 rank=(b * n * c * (m + 1), torch.int32, ISENTINEL), pixel=(n * b * c * h * w * 4, torch.float32, SENTINEL))
    outs = {k: _guarded(sz, off_out, dt, fill) + (fill,) for k, (sz, dt, fill) in sizes.items()}
    want = dict(scores=True, seq=seq, rank=rank, pixel=pixel)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.lns_op_ensemble_score(ins[0].data_ptr(), ins[1].data_ptr(), n, b, m, c, h, w, ctypes.byref(spec),
                                 *[outs[k][1].data_ptr() if want[k] else None for k in ("scores", "seq", "rank", "pixel")], stream)
    assert rc == expect, (rc, L.lns_create_error())
    torch.cuda.synchronize()
    for k, (buf, view, fill) in outs.items():
        lo = 4 + off_out
        assert bool((buf[:lo] == fill).all()) and bool((buf[lo + view.numel():] == fill).all()), k
        if not want[k] or rc != 0:
            assert bool((buf == fill).all()), k
    return (outs["scores"][1].view(b, n, c, 4), outs["seq"][1].view(b, c, 4), outs["rank"][1].view(b, n, c, m + 1),
            outs["pixel"][1].view(n, b, c, h, w, 4))


SHAPES = [(b, n, c, hw) for b in (1, 3) for n in (1, 2) for c in (1, 3) for hw in ((1, 1), (3, 5), (16, 16), (17, 16), (61, 121))]


@pytest.mark.parametrize("m", [2, 3, 33, 128])
def test_op_has_the_bits_of_the_statement(m):
    """B in {1, 3} x n in {1, 2} x C in {1, 3} x H x W in {1x1, 3x5, 16x16 (exactly one pass of the block), 17x16 (one pass and
    a tail), 61x121} with the scalar spec, and 3x5 and 61x121 again with the per-channel spec (walls, clamp), each with
    aligned inputs and with frames / y one float off a 16-byte boundary: per pixel mu, var, crps, rank; per plane the rank
    histogram, the four scores and the sequence-wise scores; nothing written outside the outputs.  The statement is
    evaluated once for all the shapes of one M (it is elementwise: the pixels are concatenated)."""
    _need_gpu()
    g = torch.Generator(device="cuda")
    g.manual_seed(100 + m)
    cases = []
    for (b, n, c, (h, w)) in SHAPES:
        for norm in (SCALAR,) + ((per_channel_norm(c),) if (h, w) in ((3, 5), (61, 121)) else ()):
            frames = torch.randn((n, b, m, c, h, w), device="cuda", generator=g) * 1.5 + 0.25
            y = torch.randn((b, n, c, h, w), device="cuda", generator=g) * 1.5 + 0.25
            v = ref.denorm(frames, norm).permute(2, 0, 1, 3, 4, 5).reshape(m, -1)
            q = ref.denorm(y, norm).permute(1, 0, 2, 3, 4).reshape(-1)
            cases.append((frames, y, norm, v, q))
    mu, var, crps, rank = ref.pixels32(torch.cat([c[3] for c in cases], 1), torch.cat([c[4] for c in cases]))
    at = 0
    for frames, y, norm, v, q in cases:
        n, b, _, c, h, w = frames.shape
        shp = (n, b, c, h, w)
        sl = slice(at, at + q.numel())
        at += q.numel()
        r_mu, r_var, r_crps, r_rank, qq = mu[sl].view(shp), var[sl].view(shp), crps[sl].view(shp), rank[sl].view(shp), q.view(shp)
        want_pixel = torch.stack([r_mu, r_var, r_crps, r_rank.float()], -1)
        want_hist = ref.rank_histogram(r_rank, m).int()
        want_scores, want_seq, _ = ref.plane_scores32(r_mu, r_var, r_crps, qq, 1e-8)
        assert bool((want_hist.sum(-1) == h * w).all())
        for offs in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
            scores, seq, hist, pixel = _op(frames, y, norm, *offs)
            tag = (m, shp, "per_channel" if norm is not SCALAR else "scalar", offs)
            assert _same(pixel, want_pixel), tag
            assert torch.equal(hist, want_hist), tag
            assert _same(scores, want_scores) and _same(seq, want_seq), tag
    # only the scores asked for: the other outputs stay untouched, the scores are the same
    frames, y, norm = cases[-1][:3]
    scores2, _, _, _ = _op(frames, y, norm, rank=False, seq=False, pixel=False)
    assert _same(scores2, _op(frames, y, norm)[0])


def _rule(ours, own, want, what, gate=True):
    """max(2e-7, 3 x own) against float64, in both measures -> the two ratios ours / bound."""
    def errs(a):
        d = a.double() - want
        return float(d.abs().max() / want.abs().max()), float(d.norm() / want.norm())
    o, w = errs(ours), errs(own)
    ratios = [a / max(FLOOR, 3.0 * b) for a, b in zip(o, w)]
    print("%s: rel-max %.3e (own %.3e) rel-L2 %.3e (own %.3e) -> %.3f %.3f of the bound%s"
          % (what, o[0], w[0], o[1], w[1], ratios[0], ratios[1], "" if gate else "  (printed, not gated)"))
    if gate:
        assert o[0] <= max(FLOOR, 3.0 * w[0]) and o[1] <= max(FLOOR, 3.0 * w[1]), (what, o, w)
    return ratios


def _fields(b, n, m, c, h, w, g):
    return torch.randn((n, b, m, c, h, w), device="cuda", generator=g), torch.randn((b, n, c, h, w), device="cuda", generator=g)


def _score_against_float64(frames, y, norm, what, gated=NAMES):
    """Plane sums (the statement's order on the kernel's own per-pixel values, which test_op_has_the_bits_of_the_statement
    ties to the kernel's sums) and the finished scores of the op against scores64 under the rule; ranks exactly."""
    m = frames.shape[2]
    scores, seq, hist, pixel = _op(frames, y, norm)
    want = ref.scores64(frames, y, **norm)
    own = ref.scores32_torch(frames, y, **norm)
    q = ref.denorm(y, norm).permute(1, 0, 2, 3, 4)
    s2, q2, sums = ref.plane_scores32(pixel[..., 0], pixel[..., 1], pixel[..., 2], q, float(norm.get("eps", 1e-8)))
    assert _same(scores, s2) and _same(seq, q2), what
    for k, score in (("SE", "rmse"), ("G", None), ("V", "spread"), ("CR", "crps")):      # (G is the truth alone: always held)
        _rule(sums[k], own[k], want[k], "%s sum %s" % (what, k), gate=score is None or score in gated)
    for i, name in enumerate(NAMES):
        _rule(scores[..., i], own["scores"][..., i], want["scores"][..., i], "%s %s" % (what, name), gate=name in gated)
        _rule(seq[..., i], own["seq"][..., i], want["seq"][..., i], "%s seq %s" % (what, name), gate=name in gated)
    return scores, seq, hist, pixel, want


@pytest.mark.parametrize("m", [2, 7, 33])
def test_op_scores_against_float64(m):
    """B = 2, n = 2, C = 3, 23 x 29 pixels (two passes and a tail).  Inputs: normal, 1e-12 x and 1e12 x (identity spec, so
    the scale is the scale of what is squared and summed), and normal with the scalar spec.  Members at 1e3 + 1e-2 x
    normal with the truth drawn likewise: only spread, crps and the ranks are held to the rule -- mu - q cancels to the
    rounding of a sum at 1e3, in torch as here, so rmse and rel_l2 are printed and not gated.  Every case prints its ratios.
    Measured on MI355X, ours / max(2e-7, 3 x own) as (rel-max, rel-L2), worst over M in {2, 7, 33} and over the sums, scores and
    sequence-wise scores: normal 0.510, 0.343; normal with the scalar spec 0.450, 0.277; 1e-12 0.579, 0.338; 1e12 0.529, 0.309;
    1e3 + 1e-2 gated (spread, crps, V, CR, G) 0.421, 0.249 -- its spread at 3e-8 against torch.var's own 7e-5 -- and printed
    (rmse, rel_l2: 6e-4 against torch's own 5e-4) 0.601, 0.585; equal members 0.441, 0.333."""
    _need_gpu()
    g = torch.Generator(device="cuda")
    g.manual_seed(200 + m)
    b, n, c, h, w = 2, 2, 3, 23, 29
    base_f, base_y = _fields(b, n, m, c, h, w, g)
    ident = dict(mean=0.0, std=1.0, eps=1e-30)
    for what, frames, y, norm, gated in (
            ("normal", base_f, base_y, ident, NAMES), ("normal scalar spec", base_f, base_y, SCALAR, NAMES),
            ("1e-12", 1e-12 * base_f, 1e-12 * base_y, ident, NAMES),
            ("1e12", 1e12 * base_f, 1e12 * base_y, ident, NAMES),
            ("1e3 + 1e-2", 1e3 + 1e-2 * base_f, 1e3 + 1e-2 * base_y, ident, ("spread", "crps"))):
        frames, y = frames.contiguous(), y.contiguous()
        scores, seq, hist, pixel, want = _score_against_float64(frames, y, norm, "M=%d %s" % (m, what), gated)
        if norm is not SCALAR:                         # the identity map is exact: float64 sees the same comparisons
            assert torch.equal(hist.long(), want["rank"]), what
        assert bool((hist.sum(-1) == h * w).all())
    # all members equal, values rounded to bfloat16: every partial sum k * v, k <= 33, is exact in fp32 (8 + 6 bits), so mu is v,
    # every d_m is 0 and the spread is exactly 0; crps is then the mean |v - q| and rmse its root-mean-square
    v = base_f[:, :, :1].to(torch.bfloat16).to(torch.float32).expand(n, b, m, c, h, w).contiguous()
    scores, seq, hist, pixel, want = _score_against_float64(v, base_y, ident, "M=%d equal members" % m, ("rel_l2", "rmse", "crps"))
    assert bool((scores[..., 2] == 0).all()) and bool((seq[..., 2] == 0).all()) and bool((pixel[..., 1] == 0).all())
    assert _same(pixel[..., 0], v[:, :, 0])
    err = (v[:, :, 0].double() - base_y.double().permute(1, 0, 2, 3, 4)).abs()
    assert torch.allclose(scores[..., 3].double(), err.mean((-2, -1)).permute(1, 0, 2), rtol=1e-5, atol=0)
    assert torch.allclose(scores[..., 1].double(), (err ** 2).mean((-2, -1)).sqrt().permute(1, 0, 2), rtol=1e-5, atol=0)


def test_op_ties_nonfinite_members_and_refused_member_counts():
    _need_gpu()
    from lns_amd import _lib
    g = torch.Generator(device="cuda")
    g.manual_seed(31)
    b, n, m, c, h, w = 2, 2, 5, 2, 9, 31
    frames, y = _fields(b, n, m, c, h, w, g)
    # ties: member 1 IS the truth (never counted: the rank follows <), member 3 equals member 0
    tied = frames.clone()
    tied[:, :, 1] = y.permute(1, 0, 2, 3, 4)
    tied[:, :, 3] = tied[:, :, 0]
    scores, seq, hist, pixel = _op(tied, y, SCALAR)
    r_mu, r_var, r_crps, r_rank = ref.statement32(tied, y, **SCALAR)
    assert _same(pixel, torch.stack([r_mu, r_var, r_crps, r_rank.float()], -1))
    assert torch.equal(hist, ref.rank_histogram(r_rank, m).int()) and bool((hist[..., m] == 0).all())
    v = ref.denorm(tied, SCALAR)
    q = ref.denorm(y, SCALAR).permute(1, 0, 2, 3, 4)
    assert torch.equal(pixel[..., 3].long(), sum((v[:, :, k] < q).long() for k in (0, 2, 3, 4)))
    # one NaN in one member of one pixel: that plane's four scores (and its sequence-wise ones) are NaN, every other plane is
    # finite, and the NaN member is not counted in the rank.  An inf likewise makes its plane non-finite and no other: SE and a
    # become inf (rel_l2, rmse = inf), the deviations inf - inf (spread, crps = NaN).
    for bad, every_nan in ((float("nan"), True), (float("inf"), False), (float("-inf"), False)):
        f2 = frames.clone()
        f2[1, 1, 2, 0, 4, 17] = bad                                       # step 1, trajectory 1, member 2, channel 0
        scores, seq, hist, pixel = _op(f2, y, SCALAR)
        hit = torch.zeros((b, n, c), dtype=torch.bool, device="cuda")
        hit[1, 1, 0] = True
        assert torch.equal(~torch.isfinite(scores).any(-1), hit) and torch.equal(~torch.isfinite(scores).all(-1), hit), bad
        assert torch.equal(~torch.isfinite(seq).all(-1), hit.any(1)), bad
        if every_nan:
            assert bool(torch.isnan(scores[1, 1, 0]).all()) and bool(torch.isnan(seq[1, 0]).all())
        r_rank = ref.statement32(f2, y, **SCALAR)[3]
        assert torch.equal(hist, ref.rank_histogram(r_rank, m).int()) and bool((hist.sum(-1) == h * w).all())
        clean = ref.statement32(frames, y, **SCALAR)[3]
        changed = (r_rank != clean).nonzero()
        assert changed.shape[0] <= 1                                      # at most the one pixel's rank moved
    # M = 1 and M = 129 are refused before any launch
    for mm in (1, 129):
        f1, y1 = _fields(1, 1, mm, 1, 2, 2, g)
        _op(f1, y1, SCALAR, expect=_lib.LNS_EINVAL)
        assert "M in 2 .. 128" in _lib.lib().lns_create_error().decode()


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
        return SCALAR
    return dict(mean=[0.1 * c for c in range(args.in_channels)], std=[1.0 + 0.5 * c for c in range(args.in_channels)])


def _case(name):
    """(args, model, engine, x, z [B, M, c, h, w], param [B, M] or None, norm, {steps: reference}) -- built once per preset,
    as tests/test_rollout_ensemble_gpu.py does; never written afterwards."""
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
        _cases[name] = (args, model, eng, xd, z, pd, _case_norm(args), {})
    return _cases[name]


def _ref(name, steps):
    """-> (member frames [steps, B, M, C, Ly, Lx] from rollout_latent at batch B * M, the truth y [B, steps, C, Ly, Lx],
    {keep: what the op and rollout_latent_ensemble give for it})."""
    args, model, eng, xd, z, pd, norm, refs = _case(name)
    if steps not in refs:
        from lns_amd import filler
        _options(eng)
        full, _ = eng.rollout_latent(z.view((B * M,) + tuple(z.shape[2:])), steps, param=None if pd is None else pd.reshape(-1))
        torch.cuda.synchronize()
        frames = full.view((B, M) + tuple(full.shape[1:])).permute(2, 0, 1, 3, 4, 5).contiguous()
        # a truth near the forecast (the control member plus noise of the members' scale), so that ranks fall on both sides
        g = torch.Generator(device="cuda")
        g.manual_seed(steps)
        y = (frames[:, :, 0].permute(1, 0, 2, 3, 4) + 0.02 * torch.randn(full[:B].shape, device="cuda", generator=g)).contiguous()
        refs[steps] = (frames, y, {})
    return refs[steps]


def _want(name, steps, keep):
    args, model, eng, xd, z, pd, norm, _ = _case(name)
    frames, y, per_keep = _ref(name, steps)
    k = tuple(keep)
    if k not in per_keep:
        _options(eng)
        op = eng.ensemble_score(frames[keep].contiguous(), y[:, keep].contiguous(), **norm)
        mean, var, z_last = eng.rollout_latent_ensemble(z, steps, param=pd, keep_steps=keep, return_last=True)
        torch.cuda.synchronize()
        per_keep[k] = (op, mean, var, z_last)
    return per_keep[k]


def _check(name, steps, keep, twice=False, outputs=True):
    args, model, eng, xd, z, pd, norm, _ = _case(name)
    opts = dict(eng.options)
    op, mean, var, z_last = _want(name, steps, keep)
    _options(eng, **{k: opts.get(k, DEFAULTS[k]) for k in DEFAULTS})
    y = _ref(name, steps)[1]
    for _ in range(2 if twice else 1):
        got = eng.rollout_latent_ensemble_eval(z, y, steps, param=pd, keep_steps=keep, return_mean=outputs, return_var=outputs,
                                               return_last=outputs, **norm)
        torch.cuda.synchronize()
        tag = (name, keep, eng.options)
        assert got.rel_l2.shape == (B, len(keep), args.in_channels) and got.rank.shape == (B, len(keep), args.in_channels, M + 1)
        for field in NAMES + ("seq",):
            assert _same(getattr(got, field), getattr(op, field)), (field,) + tag
        assert torch.equal(got.rank, op.rank), tag
        assert bool((got.rank.sum(-1) == args.Ly * args.Lx).all())
        if outputs:
            assert _same(got.mean, mean) and _same(got.var, var) and _same(got.z_last, z_last), tag
        else:
            assert got.mean is None and got.var is None and got.z_last is None
    return got


GRID = [("ns2d_mini", dg, ds, ov) for dg in (1, 2, 3, 0) for ds in (1, 3) for ov in (0, 1)] + \
       [(c, dg, ds, 1) for c in ("twophase_cond", "sw_half_periodic") for dg in (1, 2) for ds in (1, 3)]


@pytest.mark.parametrize("case,dg,ds,ov", GRID)
def test_engine_scores_have_the_bits_of_the_op_on_the_member_rollouts(case, dg, ds, ov):
    """scores, seq and rank of the call == lns_op_ensemble_score on rollout_latent(z.view(B * M, ...), T)[:, keep] arranged as
    [n][B][M], bit for bit, for every scheduling option; mean, var and z_last are rollout_latent_ensemble's bits.
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


def test_scores_alone_twice_and_with_reused_ring_groups_and_frame_buffers():
    """Without mean / var / z_last (no reduction launch) the scores are the same; twice in a row on one workspace; and the
    two keep sets of tests/test_rollout_ensemble_gpu.py::test_ring_groups_and_frame_buffers_are_reused (more kept groups
    than ring groups, and than frame buffers: a frame buffer is scored before the next decode on its stream overwrites it)."""
    _need_gpu()
    eng = _case("ns2d_mini")[2]
    ds = 3
    ngroup = ds + 2
    try:
        _options(eng)
        _check("ns2d_mini", T, [1, 4, 6], twice=True, outputs=False)
        _check("ns2d_mini", T, [1, 4, 6], twice=True)
        _options(eng, decode_group=1, decode_streams=ds)
        _check("ns2d_mini", 12, [0, 2, 3, 7, 8, 11], twice=True)
        steps = 2 * ngroup + 4
        keep2 = [t for t in range(steps) if t not in (1, 5, 6)]
        assert len(keep2) == 2 * ngroup + 1
        _check("ns2d_mini", steps, keep2, twice=True)
    finally:
        _options(eng)


def test_check_finite_and_diagnostic_modes_after_a_scored_ensemble_rollout():
    _need_gpu()
    args, model, eng, xd, z, pd, norm, _ = _case("ns2d_mini")
    keep = [1, 4, 6]
    _want("ns2d_mini", T, keep)
    try:
        for opts in (dict(), dict(decode_group=2), dict(overlap=0)):
            _options(eng, **opts)
            _check("ns2d_mini", T, keep)
            eng.check_finite(B * M, z.device)                    # LNS_OK: raises otherwise
        _options(eng, decode_group=2)
        eng.set_option("track_nonfinite", 1)
        _check("ns2d_mini", T, keep)
        eng.check_finite(B * M)
        eng.set_option("track_nonfinite", 0)
        eng.timing_enable(True)                                  # diagnostics modes: everything on the caller's stream
        _check("ns2d_mini", T, keep)
        eng.timing_enable(False)
        eng.trace_enable(True)
        _check("ns2d_mini", T, keep)
        eng.trace_enable(False)
    finally:
        eng.timing_enable(False)
        eng.trace_enable(False)
        eng.set_option("track_nonfinite", 0)
        _options(eng)


def test_workspace_is_the_ensemble_rollouts_and_a_short_one_is_refused():
    _need_gpu()
    from lns_amd import _lib, engine
    args, model, eng, xd, z, pd, norm, _ = _case("ns2d_mini")
    L, h = eng._L, eng._h
    keep = [1, 4, 6]
    op, mean_ref, var_ref, _ = _want("ns2d_mini", T, keep)
    y = _ref("ns2d_mini", T)[1][:, keep].contiguous()
    _options(eng)
    n1 = ctypes.c_size_t(0)
    assert L.lns_rollout_ensemble_workspace_bytes(h, B, M, ctypes.byref(n1)) == 0
    C = args.in_channels
    scores = torch.full((B, 3, C, 4), SENTINEL, device="cuda")
    seq = torch.full((B, C, 4), SENTINEL, device="cuda")
    rank = torch.full((B, 3, C, M + 1), ISENTINEL, dtype=torch.int32, device="cuda")
    mean = torch.full((B, 3, C, args.Ly, args.Lx), SENTINEL, device="cuda")
    var = torch.full_like(mean, SENTINEL)
    last = torch.full_like(z, SENTINEL)
    ws = torch.empty(n1.value, dtype=torch.uint8, device="cuda")
    spec = engine.eval_spec(C, **norm)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run(nbytes):
        return L.lns_rollout_latent_ensemble_eval(h, z.data_ptr(), None, y.data_ptr(), B, M, T, (ctypes.c_int * 3)(*keep), 3,
                                                  ctypes.byref(spec), scores.data_ptr(), seq.data_ptr(), rank.data_ptr(), mean.data_ptr(),
                                                  var.data_ptr(), last.data_ptr(), ws.data_ptr(), nbytes, stream)
    assert run(n1.value - 1) == _lib.LNS_ENOMEM and "ensemble workspace too small" in L.lns_last_error(h).decode()
    torch.cuda.synchronize()
    for t, fill in ((scores, SENTINEL), (seq, SENTINEL), (rank, ISENTINEL), (mean, SENTINEL), (var, SENTINEL), (last, SENTINEL)):
        assert bool((t == fill).all())                                       # nothing was enqueued
    assert run(n1.value) == 0                                                # exactly the ensemble rollout's workspace
    torch.cuda.synchronize()
    assert _same(scores[..., 0], op.rel_l2) and _same(scores[..., 3], op.crps) and _same(seq, op.seq) and torch.equal(rank, op.rank)
    assert _same(mean, mean_ref) and _same(var, var_ref)


# ---- validate_ensemble ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["ns2d_mini", "twophase_cond"])
def test_validate_ensemble_is_the_hand_written_composition(case):
    """x_to_z, randn with the same generator state, rollout_latent_ensemble_eval: equal bits; reproducible with the generator
    reset; with 8 free members the spread-skill ratio is finite and positive."""
    _need_gpu()
    from lns_amd import metrics
    args, model, eng, xd, z, pd, norm, _ = _case(case)
    _options(eng)
    y = _ref(case, T)[1]
    members, keep = 4, [0, 3, 6]
    extra = (pd[:, 0].contiguous(),) if pd is not None else ()          # [B]: shared by a trajectory's members
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    got = model.validate_ensemble(xd, y, *extra, members, NOISE, generator=g, keep_steps=keep, **norm)
    g.manual_seed(5)
    z0 = model.x_to_z(xd)
    eps = torch.randn((B, members) + tuple(z0.shape[1:]), device=z0.device, generator=g) * NOISE
    zz = z0[:, None] + eps
    zz[:, 0] = z0
    param = extra[0][:, None].expand(B, members).contiguous() if extra else None
    hand = eng.rollout_latent_ensemble_eval(zz, y, param=param, keep_steps=keep, **norm)
    g.manual_seed(5)
    again = model.validate_ensemble(xd, y, *extra, members, NOISE, generator=g, keep_steps=keep, **norm)
    free = model.validate_ensemble(xd, y, *extra, 8, NOISE, generator=g, control=False, keep_steps=keep, **norm)
    torch.cuda.synchronize()
    for field in NAMES + ("seq",):
        assert _same(getattr(got, field), getattr(hand, field)) and _same(getattr(got, field), getattr(again, field)), field
    assert torch.equal(got.rank, hand.rank) and torch.equal(got.rank, again.rank)
    assert got.mean is None and got.var is None and got.z_last is None
    ratio = metrics.spread_skill_ratio(free, 8)
    assert ratio.shape == (B, len(keep), args.in_channels)
    # (a clamped channel can have every member at a bound, spread 0: the ratio is held on the others)
    free_c = torch.tensor([c not in norm.get("clamp_channels", ()) for c in range(args.in_channels)], device="cuda")
    assert bool(torch.isfinite(ratio[..., free_c]).all()) and bool((ratio[..., free_c] > 0).all())
    assert _same(ratio, free.spread * float(9 / 8) ** 0.5 / free.rmse)


def test_validate_ensemble_without_noise_is_the_control():
    """noise_level = 0 with two members (2 v / 2 is exactly v; a third member would round 3 v): the spread is exactly 0, crps
    is the mean absolute error of the control and rel_l2 is validate(...)'s frame-wise value for the kept steps -- the latter
    under the rule max(2e-7, 3 x own), not bits: metric_plane_sums forms the error as (p - q) * sd, the statement here as
    D(p) - D(q).  `own` is validate's own distance from the float64 value.  Measured on MI355X (rel-max, rel-L2 of the bound):
    crps 0.263, 0.218; rel_l2 0.282, 0.170."""
    _need_gpu()
    args, model, eng, xd, z, pd, norm, _ = _case("ns2d_mini")
    _options(eng)
    y = _ref("ns2d_mini", T)[1]
    keep = [0, 3, 6]
    got = model.validate_ensemble(xd, y, 2, 0.0, keep_steps=keep, **norm)
    frame, _, _ = model.validate(xd, y, **norm)
    pred = model.predict(xd, T, to_x=True)[:, keep]
    torch.cuda.synchronize()
    assert bool((got.spread == 0).all()) and bool((got.seq[..., 2] == 0).all())
    assert bool((got.rank[..., 1] == 0).all())                           # both members on the same side of the truth
    p64 = pred.double() * float(np.float32(norm["std"])) + float(np.float32(norm["mean"]))
    q64 = y[:, keep].double() * float(np.float32(norm["std"])) + float(np.float32(norm["mean"]))
    mae = (p64 - q64).abs().mean((-2, -1))
    own_mae = (ref.denorm(pred, norm) - ref.denorm(y[:, keep], norm)).abs().mean((-2, -1))
    _rule(got.crps, own_mae, mae, "crps against the mean absolute error")
    want = ((p64 - q64) ** 2).sum((-2, -1)).sqrt() / (q64 ** 2).sum((-2, -1)).sqrt()
    _rule(got.rel_l2, frame[:, keep], want, "rel_l2 against validate's frame-wise value")

"""GPU (-m gpu): the ensemble transform Kalman filter (lns_op_ensemble_obs_gram, lns_op_etkf_transform,
lns_op_ensemble_transform, lns_rollout_latent_ensemble_analysis, include/lns.h; Engine.ensemble_obs_gram / etkf_transform /
ensemble_transform / rollout_latent_ensemble_analysis, enkf.EnsembleFilter, LatentDynamics.assimilate_ensemble).

The Gram sums and the transform are held to the project's rule against tests/etkf_reference.py: max(1e-12, 3 x own) in rel-L2
and in max|diff| / max|ref|, own = the reference's float64 form against its longdouble form on the same inputs.  The update
is held bit for bit to the float64 numpy statement.  The engine call is held bit for bit to the three ops applied to the
member fields that `rollout_latent` at batch B * M with keep_steps produces, over the scheduling grid.  RATIOS collects the
worst ratio to the bound per case (tools/etkf_parity.py writes it to profiles/etkf_parity.json)."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import etkf_reference as er  # noqa: E402
from ensemble_exceed_reference import SCALAR, per_channel_norm  # noqa: E402
from helpers import load_golden, case_args  # noqa: E402

pytestmark = pytest.mark.gpu

B, M, T = 2, 3, 7
NOISE = 0.05
RHO = 1.3
KEEP_SETS = ([0], [6], [1, 4, 6], [0, 1, 2, 3, 4, 5, 6], [2, 3], [0, 2, 3, 4, 6])     # tests/test_rollout_ensemble_gpu.py's
DEFAULTS = dict(decode_group=1, decode_streams=3, overlap=1)
DSENTINEL = -12345.0
RATIOS = {}                                           # case -> worst ratio to the bound (tools/etkf_parity.py)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from lns_amd import _lib
    assert _lib.lib().lns_build_has(b"ensemble_etkf") == 1


def _same(a, b):
    """equal bits, or NaN on both sides"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    a, b = a.contiguous(), b.contiguous()
    it = torch.int64 if a.dtype == torch.float64 else torch.int32
    return bool(((a.view(it) == b.view(it)) | (torch.isnan(a) & torch.isnan(b))).all())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _guarded(n, dtype=torch.float64, fill=DSENTINEL):
    """(buffer, view): n elements between four guard elements on either side, everything pre-filled with a sentinel"""
    buf = torch.full((n + 8,), fill, dtype=dtype, device="cuda")
    return buf, buf[4:4 + n]


def _guards_intact(buf, n, fill=DSENTINEL):
    return bool((buf[:4] == fill).all()) and bool((buf[4 + n:] == fill).all())


def _placed(t, off):
    """a copy of `t` that starts `off` floats behind a 16-byte boundary"""
    buf = torch.empty(t.numel() + 4, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + t.numel()]
    view.copy_(t.reshape(-1))
    return view


# ---- the Gram op ---------------------------------------------------------------------------------------------------------------
def _gram_op(frames, y, rinv, r_bs, r_ss, norm, off=0, expect=0):
    """lns_op_ensemble_obs_gram through ctypes: inputs optionally one float off a 16-byte boundary, the three outputs pre-filled
    with a sentinel between guard words that must survive; called twice, the second call must give the first one's bits."""
    from lns_amd import _lib, engine
    L = _lib.lib()
    n, b, m, c, h, w = frames.shape
    spec = engine.eval_spec(c, **norm) if norm else None
    src, obs, rv = _placed(frames, off), _placed(y, off), _placed(rinv, off)
    outs = []
    for _ in range(2):
        bufs = [_guarded(b * n * k) for k in (m * m, m, 3)]
        rc = L.lns_op_ensemble_obs_gram(src.data_ptr(), obs.data_ptr(), rv.data_ptr(), r_bs, r_ss, n, b, m, c, h, w,
                                        ctypes.byref(spec) if spec is not None else None, bufs[0][1].data_ptr(), bufs[1][1].data_ptr(),
                                        bufs[2][1].data_ptr(), _stream())
        assert rc == expect, (rc, L.lns_create_error())
        torch.cuda.synchronize()
        for (buf, view), k in zip(bufs, (m * m, m, 3)):
            assert _guards_intact(buf, b * n * k)
            assert rc != 0 or not bool((view == DSENTINEL).any())
        outs.append([v for _, v in bufs])
    for u, v in zip(*outs):
        assert _same(u, v)
    S, g, stat = outs[0]
    return S.view(b, n, m, m).cpu().numpy(), g.view(b, n, m).cpu().numpy(), stat.view(b, n, 3).cpu().numpy()


PLANES = ((1, 1), (1, 7), (3, 5), (17, 16), (61, 121))


def _gram_combos(m, h, w):
    """the eight (B, n, C) shapes of one (M, plane), each with its own family, weight-map sharing, norm, alignment and special
    inputs: q cycles the four families, shared / per-sample / per-step maps, no / scalar / per-channel norm; odd q: inputs one
    float off a 16-byte boundary and NaN / +-inf wherever rinv = 0; q = 2: a single observed value; q = 5: identical members."""
    q = 0
    for b in (1, 3):
        for n in (1, 2):
            for c in (1, 3):
                yield q, b, n, c
                q += 1


@pytest.mark.parametrize("hw", PLANES, ids=lambda p: "%dx%d" % p)
@pytest.mark.parametrize("m", [2, 3, 7, 33, 64])
def test_gram_op_under_the_rule(m, hw):
    """M x plane over B in {1, 3} x n in {1, 2} x C in {1, 3}; see _gram_combos for what each shape carries.  S, g and stat each
    within max(1e-12, 3 x own) of the longdouble statement in both distances; S symmetric to the bit; the count exact; the
    reference sees the clean inputs, the device NaN / inf at the unobserved values."""
    _need_gpu()
    h, w = hw
    worst = 0.0
    for q, b, n, c in _gram_combos(m, h, w):
        family = er.FAMILIES[q % 4][0]
        fr, yy = er.family_inputs((n, b, m, c, h, w), 1000 * m + 7 * h + w + q, family)
        per_sample, per_step = bool(q & 1), bool(q & 2)
        density = 0.25 if h * w > 1000 else 0.6
        r = er.rinv_map((b, n, c, h, w), 50 + q + m, density=density, per_sample=per_sample, per_step=per_step)
        if q == 2:
            r = np.zeros_like(r)
            r.reshape(-1)[r.size // 2] = 1.5
        if q == 5:
            fr = np.ascontiguousarray(np.broadcast_to(fr[:, :, :1], fr.shape))
        norm = (None, SCALAR, per_channel_norm(c))[q % 3]
        per = c * h * w
        r_bs, r_ss = (n * per if per_sample else 0), (per if per_step or per_sample else 0)
        r_dev = np.ascontiguousarray(np.broadcast_to(r, (b, n, c, h, w)) if per_sample else r).copy()
        full_r = np.broadcast_to(r, (b, n, c, h, w))
        fr_dev, yy_dev = fr.copy(), yy.copy()
        if q & 1:
            hole = ~(full_r > 0)
            yy_dev[hole] = np.nan
            holes = np.broadcast_to(hole.transpose(1, 0, 2, 3, 4)[:, :, None], fr.shape)
            fr_dev[holes & (np.arange(m).reshape(1, 1, m, 1, 1, 1) % 2 == 0)] = np.inf
            fr_dev[holes & (np.arange(m).reshape(1, 1, m, 1, 1, 1) % 2 == 1)] = -np.nan
        got = _gram_op(torch.from_numpy(fr_dev).cuda(), torch.from_numpy(yy_dev).cuda(), torch.from_numpy(r_dev).cuda(), r_bs, r_ss,
                       norm, off=q & 1)
        r64, rld = er.gram(fr, yy, full_r, norm), er.gram(fr, yy, full_r, norm, dt=er.LD)
        tag = (m, h, w, q, b, n, c, family)
        for name, u, v64, vld in zip(("S", "g", "stat"), got, r64, rld):
            ok, ratio, dist, lim = er.held(u, v64, vld)
            worst = max(worst, ratio)
            assert ok, tag + (name, dist, lim)
        assert np.array_equal(got[0], got[0].transpose(0, 1, 3, 2)), tag
        assert np.array_equal(got[2][:, :, 2], (full_r > 0).sum((2, 3, 4))), tag
        if q == 5:
            assert not got[0].any() and not got[1].any(), tag
    RATIOS["gram M=%d %dx%d" % (m, h, w)] = worst
    print("gram M=%d %dx%d: worst ratio to the bound %.3g" % (m, h, w, worst))


# ---- the transform op -----------------------------------------------------------------------------------------------------------
def _transform_op(S, g, rho, expect=0):
    from lns_amd import _lib
    L = _lib.lib()
    b, n, m = g.shape
    Sd, gd = torch.from_numpy(np.ascontiguousarray(S)).cuda(), torch.from_numpy(np.ascontiguousarray(g)).cuda()
    bufs = [_guarded(b * k) for k in (m * m, m, m)] + [_guarded(b, torch.int32, -77)]
    rc = L.lns_op_etkf_transform(Sd.data_ptr(), gd.data_ptr(), b, n, m, rho, bufs[0][1].data_ptr(), bufs[1][1].data_ptr(),
                                 bufs[2][1].data_ptr(), bufs[3][1].data_ptr(), _stream())
    assert rc == expect, (rc, L.lns_create_error())
    torch.cuda.synchronize()
    for (buf, view), k in zip(bufs[:3], (m * m, m, m)):
        assert _guards_intact(buf, b * k)
    assert _guards_intact(bufs[3][0], b, -77)
    X, wbar, lam, status = (v for _, v in bufs)
    return X.view(b, m, m).cpu().numpy(), wbar.view(b, m).cpu().numpy(), lam.view(b, m).cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize("m", [2, 3, 7, 33, 64])
def test_transform_op_under_the_rule(m):
    """Grams from the reference whose A has the condition number 1, 10, 100 and 1e4, two steps each (summed in the kernel): X,
    wbar and lam within max(1e-12, 3 x own) of the longdouble statement; the residual || W A W - (M - 1) I ||_F / ((M - 1) sqrt M)
    of the device's W = X - wbar 1^T within max(1e-12, 3 x the float64 reference's); W symmetric to the bit; lam ascending;
    status 0.  One sample at M = 64 (the longdouble Jacobi of the reference takes a second per sample)."""
    _need_gpu()
    worst = 0.0
    for cond in (1.0, 10.0, 1e2, 1e4):
        S, g = er.gram_with_condition(m, cond, 10 * m + int(np.log10(cond)), B=1 if m == 64 else 2)
        X, wbar, lam, status = _transform_op(S, g, RHO)
        r64, rld = er.transform(S, g, RHO), er.transform(S, g, RHO, dt=er.LD)
        assert (status == 0).all() and (r64[3] == 0).all()
        for name, u, k in (("X", X, 0), ("wbar", wbar, 1), ("lam", lam, 2)):
            ok, ratio, dist, lim = er.held(u, r64[k], rld[k])
            worst = max(worst, ratio)
            assert ok, (m, cond, name, dist, lim)
        W = X - wbar[:, :, None]
        res, res_ref = er.residual(W, S, g, RHO), er.residual(r64[4], S, g, RHO)
        lim = max(er.FLOOR, 3.0 * res_ref.max())
        worst = max(worst, res.max() / lim)
        assert res.max() <= lim, (m, cond, res, res_ref)
        assert (np.diff(lam, axis=1) >= 0).all()
        if cond == 1.0:                                # S = 0: no rotation, X = sqrt((M - 1) / dg) I to the bit
            assert np.array_equal(X, r64[0]) and not wbar.any()
    RATIOS["transform M=%d" % m] = worst
    print("transform M=%d: worst ratio to the bound %.3g" % (m, worst))


def test_transform_marks_a_non_finite_gram_in_that_sample_only():
    """NaN in S of sample 1, inf in g of sample 3: status 1 and NaN in X, wbar, lam of those samples; samples 0 and 2 as without."""
    _need_gpu()
    m = 7
    S, g = er.gram_with_condition(m, 100.0, 3, B=4)
    clean = _transform_op(S, g, RHO)
    S2, g2 = S.copy(), g.copy()
    S2[1, 1, 2, 3] = np.nan
    g2[3, 0, 5] = np.inf
    X, wbar, lam, status = _transform_op(S2, g2, RHO)
    assert status.tolist() == [0, 1, 0, 1]
    for u, v in zip((X, wbar, lam), clean):
        assert np.isnan(u[[1, 3]]).all()
        assert np.array_equal(u[[0, 2]], v[[0, 2]])


# ---- the update op --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [2, 3, 7, 33, 64])
def test_update_op_bit_for_bit(m):
    """z [B, M, n] for B in {1, 3} and n in {1, 5, 257, 1000} (n = 1: the param update; 257: two blocks, one ragged) against the
    float64 numpy statement, bit for bit: into a separate output between guard words, in place (out aliasing z), and with z
    and out one float off a 16-byte boundary."""
    _need_gpu()
    from lns_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(m)
    for b in (1, 3):
        S, g = er.gram_with_condition(m, 100.0, m + b, B=b)
        X = er.transform(S, g, RHO, eig="eigh")[0]
        Xd = torch.from_numpy(X).cuda()
        for n in (1, 5, 257, 1000):
            z = (rng.standard_normal((b, m, n)) * 3.0 + 1.0).astype(np.float32)
            want = torch.from_numpy(er.update(z, X)).cuda()
            for off in (0, 1):
                zd = _placed(torch.from_numpy(z).cuda(), off)
                buf, out = _guarded(b * m * n + off, torch.float32)
                out = out[off:]
                assert L.lns_op_ensemble_transform(zd.data_ptr(), Xd.data_ptr(), b, m, n, out.data_ptr(), _stream()) == 0
                torch.cuda.synchronize()
                assert _guards_intact(buf, b * m * n + off) and _same(out.view(b, m, n), want), (m, b, n, off)
                assert L.lns_op_ensemble_transform(zd.data_ptr(), Xd.data_ptr(), b, m, n, zd.data_ptr(), _stream()) == 0
                torch.cuda.synchronize()
                assert _same(zd.view(b, m, n), want), (m, b, n, off, "in place")


# ---- the engine -----------------------------------------------------------------------------------------------------------------
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
    """(args, model, engine, x, z [B, M, c, h, w], param [B, M] or None, norm, y [B, T, C, Ly, Lx], rinv [B, T, C, Ly, Lx], {}) --
    built once per preset, as tests/test_rollout_ensemble_gpu.py does; never written afterwards.  The observations are the
    unperturbed rollout plus noise; about a third of the values are observed, with weights in [0.5, 2) per sample and step."""
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
        y, _ = eng.rollout_latent(z0, T, param=None if pd is None else pd[:, 0].contiguous())
        y = (y + 0.02 * y.std() * torch.randn(y.shape, device="cuda", generator=g)).contiguous()
        u = torch.rand(y.shape, device="cuda", generator=g)
        rinv = torch.where(u < 0.33, 0.5 + 4.5 * u, torch.zeros_like(u)).contiguous()
        _cases[name] = (args, model, eng, xd, z, pd, _case_norm(args), y, rinv, {})
    return _cases[name]


FIELDS = ("z", "param", "X", "wbar", "lam", "stat", "status", "mean", "var", "z_last")


def _want(name, steps, keep, with_norm=True):
    """The three ops on the member fields rollout_latent at batch B * M with keep_steps produces, and rollout_latent_ensemble's
    mean / var / z_last; computed once per (steps, keep, norm) under the default options."""
    args, model, eng, xd, z, pd, norm, y, rinv, refs = _case(name)
    key = (steps, tuple(keep), with_norm)
    if key not in refs:
        _options(eng)
        kept, zl = eng.rollout_latent(z.view((B * M,) + tuple(z.shape[2:])), steps, param=None if pd is None else pd.reshape(-1),
                                      keep_steps=keep)
        frames = kept.view((B, M) + tuple(kept.shape[1:])).permute(2, 0, 1, 3, 4, 5).contiguous()      # [n, B, M, C, Ly, Lx]
        S, g, stat = eng.ensemble_obs_gram(frames, y[:, keep].contiguous(), rinv[:, keep].contiguous(), **(norm if with_norm else {}))
        X, wbar, lam, status = eng.etkf_transform(S, g, RHO)
        za = eng.ensemble_transform(zl.view(z.shape).contiguous(), X)
        pa = eng.ensemble_transform(pd, X) if pd is not None else None
        mean, var, z_last = eng.rollout_latent_ensemble(z, steps, param=pd, keep_steps=keep, return_last=True)
        torch.cuda.synchronize()
        assert bool((status == 0).all()) and _same(z_last, zl.view(z.shape))
        refs[key] = dict(z=za, param=pa, X=X, wbar=wbar, lam=lam, stat=stat, status=status, mean=mean, var=var, z_last=z_last)
    return refs[key]


def _check(name, steps, keep, with_norm=True, outputs=True, twice=False):
    args, model, eng, xd, z, pd, norm, y, rinv, _ = _case(name)
    opts = dict(eng.options)
    want = _want(name, steps, keep, with_norm)
    _options(eng, **{k: opts.get(k, DEFAULTS[k]) for k in DEFAULTS})
    for _ in range(2 if twice else 1):
        got = eng.rollout_latent_ensemble_analysis(z, y[:, keep].contiguous(), rinv[:, keep].contiguous(), steps, param=pd, keep_steps=keep,
                                                   rho=RHO, return_mean=outputs, return_var=outputs, return_last=outputs,
                                                   **(norm if with_norm else {}))
        torch.cuda.synchronize()
        tag = (name, keep, with_norm, eng.options)
        for f in FIELDS:
            u, v = getattr(got, f), want[f]
            if f in ("mean", "var", "z_last") and not outputs:
                assert u is None, tag + (f,)
            elif v is None:
                assert u is None, tag + (f,)
            elif f == "status":
                assert torch.equal(u, v), tag + (f,)
            else:
                assert _same(u, v), tag + (f,)
    return got


GRID = [("ns2d_mini", dg, ds, 1) for dg in (1, 2, 3, 0) for ds in (1, 2, 3, 4)] + \
       [("ns2d_mini", dg, ds, 0) for dg in (1, 2, 3, 0) for ds in (1, 3)] + \
       [(c, None, None, 1) for c in ("twophase_cond", "sw_half_periodic")]


@pytest.mark.parametrize("case,dg,ds,ov", GRID)
def test_engine_call_is_the_three_ops_on_the_member_rollouts(case, dg, ds, ov):
    """z_analysis, X, wbar, lam, stat and status of the call == lns_op_ensemble_obs_gram, lns_op_etkf_transform and
    lns_op_ensemble_transform on rollout_latent(z.view(B * M, ...), T, keep_steps) arranged as [n][B][M], bit for bit, for
    every scheduling option (ns2d_mini) and at the defaults (the other two); mean, var and z_last are rollout_latent_ensemble's
    bits.  twophase_cond runs with one parameter value per member, which the same transform updates, and the per-channel spec."""
    _need_gpu()
    eng = _case(case)[2]
    try:
        for keep in KEEP_SETS:
            _want(case, T, keep)
            if dg is not None:
                _options(eng, decode_group=dg, decode_streams=ds, overlap=ov)
            got = _check(case, T, keep)
            assert (got.param is not None) == (case == "twophase_cond")
    finally:
        _options(eng)


def test_analysis_without_norm_alone_twice_and_in_the_diagnostic_modes():
    """Without a norm the values are compared as they are; without mean / var / z_last (the update then runs in place on
    z_analysis) the filter's outputs are the same; twice in a row on one workspace; more kept groups than ring groups and frame
    buffers; trace and timing modes (everything on the caller's stream); lns_check_finite covers the call; a param given per
    trajectory is not updated; rollout_latent_ensemble before and after the call returns the same bits."""
    _need_gpu()
    args, model, eng, xd, z, pd, norm, y, rinv, _ = _case("ns2d_mini")
    keep = [1, 4, 6]
    try:
        _options(eng)
        before = eng.rollout_latent_ensemble(z, T, keep_steps=keep)
        _check("ns2d_mini", T, keep, with_norm=False)
        _check("ns2d_mini", T, keep, outputs=False, twice=True)
        _check("ns2d_mini", T, keep, twice=True)
        after = eng.rollout_latent_ensemble(z, T, keep_steps=keep)
        torch.cuda.synchronize()
        assert _same(before[0], after[0]) and _same(before[1], after[1])
        eng.check_finite(B * M, z.device)
        _options(eng, decode_group=1, decode_streams=3)
        steps = 2 * 5 + 4
        keep2 = [t for t in range(steps) if t not in (1, 5, 6)]
        yy = torch.cat([y, y], 1)[:, :steps].contiguous()
        rr = torch.cat([rinv, rinv], 1)[:, :steps].contiguous()
        a = eng.rollout_latent_ensemble_analysis(z, yy[:, keep2].contiguous(), rr[:, keep2].contiguous(), steps, keep_steps=keep2, rho=RHO)
        b = eng.rollout_latent_ensemble_analysis(z, yy[:, keep2].contiguous(), rr[:, keep2].contiguous(), steps, keep_steps=keep2, rho=RHO)
        _options(eng, decode_group=3, decode_streams=1, overlap=0)
        c = eng.rollout_latent_ensemble_analysis(z, yy[:, keep2].contiguous(), rr[:, keep2].contiguous(), steps, keep_steps=keep2, rho=RHO)
        torch.cuda.synchronize()
        for f in ("z", "X", "wbar", "lam", "stat"):
            assert _same(getattr(a, f), getattr(b, f)) and _same(getattr(a, f), getattr(c, f)), f
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
    args, model, eng, xd, z, pd, norm, y, rinv, _ = _case("twophase_cond")
    shared = eng.rollout_latent_ensemble_analysis(z, y[:, keep].contiguous(), rinv[:, keep].contiguous(), T, param=pd[:, 0].contiguous(),
                                                  keep_steps=keep, rho=RHO, **norm)
    torch.cuda.synchronize()
    assert shared.param is None and bool((shared.status == 0).all())


def test_workspace_is_the_ensemble_layout_plus_one_region_and_a_short_one_is_refused():
    _need_gpu()
    from lns_amd import _lib, engine
    args, model, eng, xd, z, pd, norm, y, rinv, _ = _case("ns2d_mini")
    L, h = eng._L, eng._h
    keep = [1, 4, 6]
    want = _want("ns2d_mini", T, keep)
    _options(eng)
    n0, n1 = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert L.lns_rollout_ensemble_workspace_bytes(h, B, M, ctypes.byref(n0)) == 0
    assert L.lns_rollout_ensemble_analysis_workspace_bytes(h, B, M, 3, ctypes.byref(n1)) == 0
    assert n1.value > n0.value
    C = args.in_channels
    za = torch.full_like(z, DSENTINEL)
    X = torch.full((B, M, M), DSENTINEL, dtype=torch.float64, device="cuda")
    mean = torch.full((B, 3, C, args.Ly, args.Lx), DSENTINEL, device="cuda")
    ws = torch.empty(n1.value, dtype=torch.uint8, device="cuda")
    spec = engine.eval_spec(C, **norm)
    yk, rk = y[:, keep].contiguous(), rinv[:, keep].contiguous()
    per = C * args.Ly * args.Lx

    def run(nbytes):
        return L.lns_rollout_latent_ensemble_analysis(h, z.data_ptr(), None, yk.data_ptr(), rk.data_ptr(), 3 * per, per, B, M, T,
                                                      (ctypes.c_int * 3)(*keep), 3, ctypes.byref(spec), RHO, za.data_ptr(), None,
                                                      X.data_ptr(), None, None, None, None, mean.data_ptr(), None, None, ws.data_ptr(),
                                                      nbytes, _stream())
    for short in (n1.value - 1, n0.value):
        assert run(short) == _lib.LNS_ENOMEM and "ensemble analysis workspace too small" in L.lns_last_error(h).decode()
        torch.cuda.synchronize()
        assert bool((za == DSENTINEL).all()) and bool((X == DSENTINEL).all()) and bool((mean == DSENTINEL).all())   # nothing was enqueued
    assert run(n1.value) == 0
    torch.cuda.synchronize()
    assert _same(za, want["z"]) and _same(X, want["X"]) and _same(mean, want["mean"])


# ---- the filter and the twin experiment -----------------------------------------------------------------------------------------
def test_filter_cycles_windows_from_the_previous_analysis():
    """EnsembleFilter.run with window = 1 over two observed steps == two rollout_latent_ensemble_analysis calls by hand, the
    second from the first one's analysis; window = 2 == one call (the 4D form); dfs from lam."""
    _need_gpu()
    from lns_amd import enkf
    args, model, eng, xd, z, pd, norm, y, rinv, _ = _case("ns2d_mini")
    _options(eng)
    obs = [1, 4]
    yk, rk = y[:, obs].contiguous(), rinv[:, obs].contiguous()
    f = enkf.EnsembleFilter(model, inflation=RHO)
    got = f.run(z, yk, rk, obs, window=1, **norm)
    a = eng.rollout_latent_ensemble_analysis(z, yk[:, :1].contiguous(), rk[:, :1].contiguous(), 2, keep_steps=[1], rho=RHO, **norm)
    b = eng.rollout_latent_ensemble_analysis(a.z, yk[:, 1:].contiguous(), rk[:, 1:].contiguous(), 3, keep_steps=[2], rho=RHO, **norm)
    torch.cuda.synchronize()
    assert _same(got.z, b.z) and _same(got.X, torch.stack([a.X, b.X])) and _same(got.stat, torch.cat([a.stat, b.stat], 1))
    assert tuple(got.dfs.shape) == (2, B) and bool((got.dfs > 0).all()) and bool((got.dfs < M - 1).all()) and got.param is None
    assert torch.allclose(got.dfs[1], (1.0 - (M - 1) / (RHO * b.lam)).sum(-1), rtol=0, atol=1e-12)
    both = f.run(z, yk, rk, obs, window=2, **norm)
    one = eng.rollout_latent_ensemble_analysis(z, yk, rk, 5, keep_steps=obs, rho=RHO, **norm)
    torch.cuda.synchronize()
    assert _same(both.z, one.z) and _same(both.X[0], one.X) and tuple(both.status.shape) == (1, B)


def twin_experiment():
    """The twin experiment of tests/test_etkf_cpu.py through LatentDynamics.assimilate_ensemble (its own noise: the generator of
    the device) -> the analysis / forecast misfit per sample at the last observed step."""
    import gpu_checks as gc
    from lns_amd import filler
    t = er.TWIN
    meta, _ = load_golden(t["preset"])
    args = case_args(meta)
    model, _ = gc.build_models(args, meta["weight_seed"])
    tail = (args.in_channels, args.Ly, args.Lx)
    x0 = torch.from_numpy(filler.normal("x", (t["B"],) + tail, t["x_seed"])).cuda()
    eng = model._engine(x0)
    obs = list(t["obs_steps"])
    truth, _ = eng.rollout_latent(model.x_to_z(x0), obs[-1] + 1, keep_steps=obs)
    r = torch.from_numpy(er.twin_rinv(*tail, t["rinv"])).cuda()
    g = torch.Generator(device="cuda")
    g.manual_seed(t["gpu_seed"])
    res = model.assimilate_ensemble(x0, truth.contiguous(), obs, t["M"], t["noise_level"], rinv=r, generator=g)
    frames = model.z_to_x(res.z.reshape((-1,) + tuple(res.z.shape[2:])))
    frames = frames.view((1, t["B"], t["M"]) + tail)
    _, _, after = eng.ensemble_obs_gram(frames, truth[:, -1:].contiguous(), r)
    torch.cuda.synchronize()
    forecast = res.stat[:, -1, 0]
    return (after[:, 0, 0] / forecast).cpu().numpy(), res


def test_twin_experiment_through_assimilate_ensemble():
    """ns2d_mini, B = 2, M = 8, every 4th pixel of channel 0 observed at steps 0 and 2, one analysis per step: the weighted misfit
    of the mean of the decoded analysis members at step 2 is below that of the forecast the last analysis corrected, for every
    sample.  The float64 reference's factor for its own numpy draw: 0.401, 0.392; the device's, for the draw of its generator
    at seed 10: 0.572, 0.740 (profiles/etkf_parity.json).  The draw decides the factor (etkf_reference.TWIN), so the assertion here is
    the fall itself."""
    _need_gpu()
    ratio, res = twin_experiment()
    RATIOS["twin analysis/forecast misfit"] = ratio.tolist()
    print("twin experiment on the device: analysis / forecast misfit per sample", ratio)
    assert bool((res.status == 0).all()) and tuple(res.X.shape) == (2, er.TWIN["B"], er.TWIN["M"], er.TWIN["M"])
    assert (ratio < 1.0).all(), ratio

"""GPU (-m gpu): the ensemble exceedance tables (lns_op_ensemble_exceed, lns_rollout_latent_ensemble_exceed, include/lns.h;
Engine.ensemble_exceed / rollout_latent_ensemble_exceed, LatentDynamics.validate_exceedance, metrics.exceedance_table).

The table is integer: everything here is held by EQUALITY of every count.  The op against tests/ensemble_exceed_reference.py
(numpy comparisons and np.add.at); the engine call against the op on the member fields that `rollout_latent` at batch B * M
with keep_steps produces, over the scheduling grid."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import ensemble_exceed_reference as ref  # noqa: E402
from helpers import load_golden, case_args  # noqa: E402
SCALAR, per_channel_norm, thresholds_for, family_fields = ref.SCALAR, ref.per_channel_norm, ref.thresholds_for, ref.family_fields

pytestmark = pytest.mark.gpu

B, M, T = 2, 3, 7
NOISE = 0.05
KEEP_SETS = ([0], [6], [1, 4, 6], [0, 1, 2, 3, 4, 5, 6], [2, 3], [0, 2, 3, 4, 6])     # tests/test_rollout_ensemble_gpu.py's
DEFAULTS = dict(decode_group=1, decode_streams=3, overlap=1)
SENTINEL = -12345
FSENTINEL = -12345.0


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from lns_amd import _lib
    assert _lib.lib().lns_build_has(b"ensemble_exceed") == 1


def _same(a, b):
    """equal bits, or NaN on both sides"""
    if a.shape != b.shape:
        return False
    a, b = a.contiguous(), b.contiguous()
    return bool(((a.view(torch.int32) == b.view(torch.int32)) | (torch.isnan(a) & torch.isnan(b))).all())


# ---- the op ------------------------------------------------------------------------------------------------------------
def _guarded(n, off):
    buf = torch.full((n + 12,), SENTINEL, dtype=torch.int32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf, buf[4 + off:4 + off + n]


def _placed(t, off):
    """a copy of `t` that starts `off` floats behind a 16-byte boundary"""
    buf = torch.empty(t.numel() + 4, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + t.numel()]
    view.copy_(t.reshape(-1))
    return view


def _op(frames, y, thresholds, norm, off_in=0, off_out=0, expect=0, calls=1):
    """lns_op_ensemble_exceed through ctypes; frames and y optionally one float off a 16-byte boundary, the table optionally one
    int off; the table is pre-filled with a sentinel (every entry must be overwritten) and sits between guard words that
    must survive.  calls = 2: the op runs twice into the same table."""
    from lns_amd import _lib, engine
    L = _lib.lib()
    n, b, m, c, h, w = frames.shape
    xs = engine.exceed_spec(c, thresholds)
    spec = engine.eval_spec(c, **norm) if norm else None
    src, truth = _placed(frames, off_in), _placed(y, off_in)
    count = b * n * xs.n_thr * c * 2 * (m + 1)
    full, view = _guarded(count, off_out)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for _ in range(calls):
        rc = L.lns_op_ensemble_exceed(src.data_ptr(), truth.data_ptr(), n, b, m, c, h, w, ctypes.byref(xs),
                                      ctypes.byref(spec) if spec is not None else None, view.data_ptr(), stream)
        assert rc == expect, (rc, L.lns_create_error())
    torch.cuda.synchronize()
    lo = 4 + off_out
    assert bool((full[:lo] == SENTINEL).all()) and bool((full[lo + count:] == SENTINEL).all())
    if rc != 0:
        assert bool((full == SENTINEL).all())
    return view.view(b, n, xs.n_thr, c, 2, m + 1)


PLANES = ((1, 1), (1, 7), (3, 5), (17, 16), (61, 121))


@pytest.mark.parametrize("hw", PLANES, ids=lambda p: "%dx%d" % p)
@pytest.mark.parametrize("m", [1, 2, 3, 33, 128])
def test_op_equals_the_reference_count_for_count(m, hw):
    """B in {1, 3} x n in {1, 2} x C in {1, 3} on planes 1x1, 1x7, 3x5, 17x16 (one full tile and a ragged one), 61x121 (29 tiles),
    each without a norm, with the scalar norm and with the per-channel one (walls, clamp), with eight thresholds and with
    one; the pixels cycle through the five input families (gaussian, quantised onto the thresholds, zeros, +-inf, NaN in
    members and truth), planes below 64 pixels under every shift of the cycle.  Inputs and table at offsets 0 and 1 element;
    a sentinel table is overwritten entirely, its guard words survive, and a second call into the same table gives the
    same table.  The reference counts once per (case, norm) for eight thresholds; the single threshold is its first row."""
    _need_gpu()
    h, w = hw
    seen = np.zeros(3, dtype=bool)
    for b in (1, 3):
        for n in (1, 2):
            for c in (1, 3):
                for shift in (range(5) if b * n * c * h * w < 64 else (0,)):
                    fr, yy = family_fields((n, b, m, c, h, w), 1000 * m + 7 * h + w + shift, shift)
                    seen |= np.array([np.isnan(fr).any(), np.isinf(fr).any(), np.isnan(yy).any()])
                    frames, y = torch.from_numpy(fr).cuda(), torch.from_numpy(yy).cuda()
                    thr = thresholds_for(c)
                    for norm in (None, SCALAR, per_channel_norm(c)):
                        want = torch.from_numpy(ref.table(fr, yy, thr, norm)).cuda()
                        assert bool((want.sum((-1, -2)) == h * w).all())
                        tag = (m, b, n, c, h, w, shift, "none" if norm is None else ("scalar" if norm is SCALAR else "per_channel"))
                        for offs in ((0, 0), (1, 0), (0, 1)):
                            got = _op(frames, y, thr, norm, *offs)
                            assert torch.equal(got, want), tag + (offs,)
                        assert torch.equal(_op(frames, y, thr[:1], norm), want[:, :, :1]), tag
                        assert torch.equal(_op(frames, y, thr, norm, calls=2), want), tag
    assert h * w < 15 or seen.all()


def test_python_surfaces_and_the_shipped_probabilities():
    """Engine.ensemble_exceed is the op and metrics.exceedance_table (on the device) the statement; summed over o, the table's
    histogram over n equals bincount(round(prob * M)) of lns_op_ensemble_quantiles' prob_out on the same frames and
    thresholds."""
    _need_gpu()
    from lns_amd import metrics
    eng = _case("ns2d_mini")[2]
    for m, c, (h, w), norm in ((3, 3, (17, 16), None), (33, 3, (61, 121), per_channel_norm(3)), (128, 1, (17, 16), SCALAR),
                               (1, 3, (3, 5), per_channel_norm(3))):
        fr, yy = family_fields((2, 3, m, c, h, w), 77 + m)
        frames, y = torch.from_numpy(fr).cuda(), torch.from_numpy(yy).cuda()
        thr = thresholds_for(c)
        want = _op(frames, y, thr, norm)
        got = eng.ensemble_exceed(frames, y, thr, **(norm or {}))
        assert got.dtype == torch.int32 and torch.equal(got, want)
        stated = metrics.exceedance_table(frames.permute(1, 2, 0, 3, 4, 5).contiguous(), y, thr, **(norm or {}))
        assert stated.is_cuda and stated.dtype == torch.int32 and torch.equal(stated, want)
        prob = eng.ensemble_quantiles(frames, (), thr, **(norm or {})).prob             # [B, n, n_thr, C, H, W]
        cnt = torch.round(prob * m).to(torch.int64)
        plane = torch.arange(cnt[..., 0, 0].numel(), device="cuda").view(cnt.shape[:4] + (1, 1)) * (m + 1)
        hist = torch.bincount((plane + cnt).reshape(-1), minlength=plane.numel() * (m + 1)).view(cnt.shape[:4] + (m + 1,))
        assert torch.equal(want.sum(4, dtype=torch.int64), hist), (m, c, h, w)


def test_op_refuses_member_counts_outside_1_128():
    _need_gpu()
    from lns_amd import _lib
    frames = torch.randn((1, 1, 129, 1, 2, 2), device="cuda")
    _op(frames, torch.randn((1, 1, 1, 2, 2), device="cuda"), (0.5,), None, expect=_lib.LNS_EINVAL)
    assert "M in 1 .. 128" in _lib.lib().lns_create_error().decode()


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
    """(args, model, engine, x, z [B, M, c, h, w], param [B, M] or None, norm, y [B, T, C, Ly, Lx], thresholds, {}) -- built
    once per preset, as tests/test_rollout_ensemble_gpu.py does; never written afterwards.  The truth is the unperturbed
    rollout plus noise, and the thresholds are the median of the denormalised truth (a scalar) and its per-channel means, so
    both outcomes and several forecast values occur."""
    if name not in _cases:
        import gpu_checks as gc
        from lns_amd import filler, metrics
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
        norm = _case_norm(args)
        d = metrics._denormalise(y, **norm)
        thr = (float(d.median()), [float(d[:, :, c].mean()) for c in range(args.in_channels)])
        _cases[name] = (args, model, eng, xd, z, pd, norm, y, thr, {})
    return _cases[name]


def _want(name, steps, keep, with_norm=True):
    """What the op gives on the member fields rollout_latent at batch B * M with keep_steps produces, and
    rollout_latent_ensemble's mean / var / z_last; computed once per (steps, keep, norm) under the default options."""
    args, model, eng, xd, z, pd, norm, y, thr, refs = _case(name)
    key = (steps, tuple(keep), with_norm)
    if key not in refs:
        _options(eng)
        kept, _ = eng.rollout_latent(z.view((B * M,) + tuple(z.shape[2:])), steps, param=None if pd is None else pd.reshape(-1),
                                     keep_steps=keep)
        frames = kept.view((B, M) + tuple(kept.shape[1:])).permute(2, 0, 1, 3, 4, 5).contiguous()      # [n, B, M, C, Ly, Lx]
        yk = _truth(y, steps)[:, keep].contiguous()
        op = eng.ensemble_exceed(frames, yk, thr, **(norm if with_norm else {}))
        mean, var, z_last = eng.rollout_latent_ensemble(z, steps, param=pd, keep_steps=keep, return_last=True)
        torch.cuda.synchronize()
        assert bool((op.sum((-1, -2)) == args.Ly * args.Lx).all())
        refs[key] = (op, mean, var, z_last)
    return refs[key]


def _truth(y, steps):
    """the truth of `steps` steps: the case's T steps, repeated where a test rolls further"""
    return y if steps <= y.shape[1] else torch.cat([y] * (-(-steps // y.shape[1])), 1)[:, :steps].contiguous()


def _check(name, steps, keep, with_norm=True, outputs=True, twice=False):
    args, model, eng, xd, z, pd, norm, y, thr, _ = _case(name)
    opts = dict(eng.options)
    op, mean, var, z_last = _want(name, steps, keep, with_norm)
    _options(eng, **{k: opts.get(k, DEFAULTS[k]) for k in DEFAULTS})
    for _ in range(2 if twice else 1):
        got = eng.rollout_latent_ensemble_exceed(z, _truth(y, steps), steps, thr, param=pd, keep_steps=keep, return_mean=outputs,
                                                 return_var=outputs, return_last=outputs, **(norm if with_norm else {}))
        torch.cuda.synchronize()
        tag = (name, keep, with_norm, eng.options)
        assert tuple(got.table.shape) == (B, len(keep), len(thr), args.in_channels, 2, M + 1) and got.table.dtype == torch.int32
        assert torch.equal(got.table, op), tag
        if outputs:
            assert _same(got.mean, mean) and _same(got.var, var) and _same(got.z_last, z_last), tag
        else:
            assert got.mean is None and got.var is None and got.z_last is None
    return got


GRID = [("ns2d_mini", dg, ds, 1) for dg in (1, 2, 3, 0) for ds in (1, 2, 3, 4)] + \
       [("ns2d_mini", dg, ds, 0) for dg in (1, 2, 3, 0) for ds in (1, 3)] + \
       [(c, None, None, 1) for c in ("twophase_cond", "sw_half_periodic")]


@pytest.mark.parametrize("case,dg,ds,ov", GRID)
def test_engine_table_is_the_op_on_the_member_rollouts(case, dg, ds, ov):
    """The table of the call == lns_op_ensemble_exceed on rollout_latent(z.view(B * M, ...), T, keep_steps) arranged as
    [n][B][M], count for count, for every scheduling option (ns2d_mini) and at the defaults (the other two); mean, var and
    z_last are rollout_latent_ensemble's bits.  twophase_cond runs with one parameter value per member and the per-channel
    spec (walls, clamp)."""
    _need_gpu()
    eng = _case(case)[2]
    try:
        for keep in KEEP_SETS:
            _want(case, T, keep)
            if dg is not None:
                _options(eng, decode_group=dg, decode_streams=ds, overlap=ov)
            _check(case, T, keep)
    finally:
        _options(eng)


def test_table_without_norm_alone_twice_in_the_diagnostic_modes_and_around_quantile_calls():
    """Without a norm members and truth are compared as they are; without mean / var / z_last (no reduction launch) the table
    is the same; twice in a row on one workspace; more kept groups than ring groups and frame buffers; trace and timing
    modes (everything on the caller's stream); lns_check_finite covers the call; rollout_latent_ensemble_quantiles before
    and after the call returns the same bits."""
    _need_gpu()
    args, model, eng, xd, z, pd, norm, y, thr, _ = _case("ns2d_mini")
    keep = [1, 4, 6]
    try:
        _options(eng)
        before = eng.rollout_latent_ensemble_quantiles(z, T, (0.05, 0.5, 0.95), thr, keep_steps=keep, return_mean=True, **norm)
        _check("ns2d_mini", T, keep, with_norm=False)
        _check("ns2d_mini", T, keep, outputs=False, twice=True)
        _check("ns2d_mini", T, keep, twice=True)
        after = eng.rollout_latent_ensemble_quantiles(z, T, (0.05, 0.5, 0.95), thr, keep_steps=keep, return_mean=True, **norm)
        torch.cuda.synchronize()
        assert _same(before.quantiles, after.quantiles) and _same(before.prob, after.prob) and _same(before.mean, after.mean)
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


def test_one_member_is_the_contingency_table_of_the_rollout_itself():
    """M = 1: the table is the 2 x 2 table of the masks (rollout > thr) and (truth > thr), and CSI their IoU."""
    _need_gpu()
    from lns_amd import metrics
    args, model, eng, xd, z, pd, norm, y, thr, _ = _case("ns2d_mini")
    _options(eng)
    keep = [1, 4, 6]
    z1 = z[:, :1].contiguous()
    fields, _ = eng.rollout_latent(z1[:, 0].contiguous(), T, keep_steps=keep)
    got = eng.rollout_latent_ensemble_exceed(z1, y, T, thr, keep_steps=keep, return_mean=True)
    torch.cuda.synchronize()
    assert _same(got.mean, fields) and got.var is None
    yk = y[:, keep]
    for k, row in enumerate(ref.thresholds_per_channel(thr, args.in_channels)):
        th = torch.tensor(row, device="cuda").view(-1, 1, 1)
        f, o = fields > th, yk > th
        for oi in (0, 1):
            for ni in (0, 1):
                want = ((o == bool(oi)) & (f == bool(ni))).sum((-1, -2))
                assert torch.equal(got.table[:, :, k, :, oi, ni].long(), want), (k, oi, ni)
        iou = ((f & o).sum((-1, -2)).double() / (f | o).sum((-1, -2)).double()).cpu().numpy()
        csi = metrics.contingency_scores(got.table[:, :, k], 1).csi
        assert np.array_equal(np.nan_to_num(csi, nan=-1.0), np.nan_to_num(iou, nan=-1.0))


def test_workspace_is_the_ensemble_rollouts_and_a_short_one_is_refused():
    _need_gpu()
    from lns_amd import _lib, engine
    args, model, eng, xd, z, pd, norm, y, thr, _ = _case("ns2d_mini")
    L, h = eng._L, eng._h
    keep = [1, 4, 6]
    op, mean_ref, var_ref, _ = _want("ns2d_mini", T, keep)
    _options(eng)
    n1 = ctypes.c_size_t(0)
    assert L.lns_rollout_ensemble_workspace_bytes(h, B, M, ctypes.byref(n1)) == 0
    C = args.in_channels
    table = torch.full((B, 3, len(thr), C, 2, M + 1), SENTINEL, dtype=torch.int32, device="cuda")
    mean = torch.full((B, 3, C, args.Ly, args.Lx), FSENTINEL, device="cuda")
    var = torch.full_like(mean, FSENTINEL)
    ws = torch.empty(n1.value, dtype=torch.uint8, device="cuda")
    xs = engine.exceed_spec(C, thr)
    spec = engine.eval_spec(C, **norm)
    yk = y[:, keep].contiguous()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run(nbytes):
        return L.lns_rollout_latent_ensemble_exceed(h, z.data_ptr(), None, yk.data_ptr(), B, M, T, (ctypes.c_int * 3)(*keep), 3,
                                                    ctypes.byref(xs), ctypes.byref(spec), table.data_ptr(), mean.data_ptr(),
                                                    var.data_ptr(), None, ws.data_ptr(), nbytes, stream)
    assert run(n1.value - 1) == _lib.LNS_ENOMEM and "ensemble workspace too small" in L.lns_last_error(h).decode()
    torch.cuda.synchronize()
    assert bool((table == SENTINEL).all()) and bool((mean == FSENTINEL).all()) and bool((var == FSENTINEL).all())   # nothing was enqueued
    assert run(n1.value) == 0                                                # exactly the ensemble rollout's workspace
    torch.cuda.synchronize()
    assert torch.equal(table, op) and _same(mean, mean_ref) and _same(var, var_ref)


@pytest.mark.parametrize("case", ["ns2d_mini", "twophase_cond"])
def test_validate_exceedance_is_the_hand_written_composition(case):
    """x_to_z, randn with the same generator state, rollout_latent_ensemble_exceed: equal counts; and brier_scores of its table
    equals brier_scores of metrics.exceedance_table on the stored member rollouts."""
    _need_gpu()
    from lns_amd import metrics
    args, model, eng, xd, z, pd, norm, y, thr, _ = _case(case)
    _options(eng)
    members, keep = 4, [0, 3, 6]
    extra = (pd[:, 0].contiguous(),) if pd is not None else ()          # [B]: shared by a trajectory's members
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    got = model.validate_exceedance(xd, y, *extra, members, NOISE, thresholds=thr, generator=g, keep_steps=keep, **norm)
    g.manual_seed(5)
    z0 = model.x_to_z(xd)
    eps = torch.randn((B, members) + tuple(z0.shape[1:]), device=z0.device, generator=g) * NOISE
    zz = z0[:, None] + eps
    zz[:, 0] = z0
    param = extra[0][:, None].expand(B, members).contiguous() if extra else None
    hand = eng.rollout_latent_ensemble_exceed(zz, y, T, thr, param=param, keep_steps=keep, **norm)
    stored, _ = eng.rollout_latent(zz.reshape((B * members,) + tuple(zz.shape[2:])), T,
                                   param=None if param is None else param.reshape(-1), keep_steps=keep)
    stated = metrics.exceedance_table(stored.view((B, members) + tuple(stored.shape[1:])), y[:, keep].contiguous(), thr, **norm)
    torch.cuda.synchronize()
    assert tuple(got.table.shape) == (B, len(keep), len(thr), args.in_channels, 2, members + 1)
    assert torch.equal(got.table, hand.table) and got.mean is None and got.var is None and got.z_last is None
    assert torch.equal(got.table, stated)
    a, b = metrics.brier_scores(got.table), metrics.brier_scores(stated)
    for u, v in zip(a, b):
        assert np.array_equal(u, v, equal_nan=True)
    assert np.isfinite(a.bs).all() and (a.bs >= 0).all() and (a.bs <= 1).all()
    seq = metrics.brier_scores(got.table.sum(1, dtype=torch.int64))
    assert seq.bs.shape == (B, len(thr), args.in_channels)

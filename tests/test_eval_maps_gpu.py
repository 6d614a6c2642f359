"""GPU (-m gpu): per-pixel time maps -- time-mean, temporal variance and covariance, mean squared and largest error
(include/lns.h "time maps").

The op (lns_op_time_maps) against tests/time_maps_reference.py: BIT FOR BIT against `statement64` (the statement as a
sequential float64 torch loop), and against independent float64 reductions under the project's rule max(2e-7, 3 x own) in
both of its measures, `own` being torch's fp32 reductions.

The streaming calls (lns_rollout_eval_maps, lns_rollout_latent_eval_maps) against the op on the stored rollout, BIT FOR BIT,
for every grouping, stream count and chunking: a pixel's steps are added in ascending order by one thread per pixel, and the
accumulation launches are chained across the decode streams.  frame / seq / kept frames / spectra / statistics are held to
lns_rollout_eval_stats' bits in the same call."""
import ctypes

import pytest

torch = pytest.importorskip("torch")

import test_eval_gpu as teg  # noqa: E402
import time_maps_reference as tm  # noqa: E402

pytestmark = pytest.mark.gpu

B, T, KEEP = teg.B, teg.T, teg.KEEP
PLANES = [(1, 1), (1, 7), (3, 5), (17, 16), (23, 29), (61, 121)]
SELECTIONS = ((0, 1), (1, 2), (3, 4))
FLOOR = 2e-7
GUARD = 64
_same = teg._same


def _unaligned(t):
    """A contiguous copy of t whose base pointer is 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[1:].view(t.shape)
    v.copy_(t)
    return v


def _guarded(n, dtype, sentinel, lead):
    """-> (the n elements inside a sentinel-filled buffer, `lead` elements from its start, check())"""
    buf = torch.full((lead + n + GUARD,), sentinel, dtype=dtype, device="cuda")
    view = buf[lead:lead + n]

    def check():
        assert bool((buf[:lead] == sentinel).all()) and bool((buf[lead + n:] == sentinel).all()), "guard overwritten"
    return view, check


def _op(y_hat, y, sel=(0, 1), aligned=False, **norm):
    """lns_op_time_maps through ctypes into guarded maps and a guarded state.  Not `aligned`: inputs 4 bytes off a 16-byte
    boundary, maps at an odd element, the state 8 bytes off a 16-byte boundary (one pixel per thread); `aligned`: everything on
    16-byte boundaries (four pixels per thread where the plane allows)."""
    from lns_amd import _lib, engine
    L = _lib.lib()
    Bn, Tn, C, H, W = (int(v) for v in y.shape)
    a, g = (y_hat.contiguous(), y.contiguous()) if aligned else (_unaligned(y_hat), _unaligned(y))
    spec = engine.eval_spec(C, **norm)
    need = ctypes.c_size_t(0)
    assert L.lns_time_maps_state_bytes(Bn, C, H, W, ctypes.byref(need)) == 0
    maps, chk_m = _guarded(Bn * C * 7 * H * W, torch.float32, -7.5, GUARD if aligned else GUARD + 1)
    state, chk_s = _guarded(need.value, torch.uint8, 0xA5, GUARD if aligned else GUARD + 8)
    assert state.data_ptr() % 16 == (0 if aligned else 8)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.lns_op_time_maps(a.data_ptr(), g.data_ptr(), Bn, Tn, C, H, W, ctypes.byref(spec), sel[0], sel[1], maps.data_ptr(),
                            state.data_ptr(), need.value, stream)
    assert rc == 0, L.lns_create_error().decode()
    torch.cuda.synchronize()
    chk_m()
    chk_s()
    pad = need.value - Bn * C * H * W * 52                     # the rounding of the size is not written either
    assert pad == 0 or bool((state[need.value - pad:] == 0xA5).all())
    return maps.view(Bn, C, 7, H, W).clone()


def _specs(C):
    """The scalar spec and a per-channel one with walls on channel 0 and the clamp on the last channel."""
    scalar = dict(mean=0.37, std=1.9, eps=1e-8)
    per_ch = dict(mean=[0.4, -0.2, 0.5][:C], std=[2.1, 1.7, 0.35][:C], zero_wall_channels=(0,), clamp_channels=(C - 1,),
                  clamp=(0.0, 1.0 + 1e-8))
    return (("scalar", scalar), ("per_channel", per_ch))


def _assert_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == torch.float32, what
    diff = (got.view(torch.int32) != want.view(torch.int32)).nonzero()
    assert diff.numel() == 0, (what, diff[:4].tolist(), got[tuple(diff[0])].item(), want[tuple(diff[0])].item())


@pytest.mark.parametrize("plane", PLANES, ids=lambda p: "%dx%d" % p)
def test_op_has_the_bits_of_the_statement(plane):
    """One pixel (1x1), a row (1x7), less than a wave (3x5), a tail past 256 and a multiple of four (17x16: the four-pixel form
    when aligned), odd planes of several blocks (23x29, 61x121)."""
    teg._need_gpu()
    H, W = plane
    g = torch.Generator(device="cuda").manual_seed(1000 * H + W)
    for Bn in (1, 3):
        for Tn in (1, 2, 5, 9):
            for C in (1, 3):
                y = torch.randn((Bn, Tn, C, H, W), device="cuda", generator=g)
                y_hat = y + 0.3 * torch.randn((Bn, Tn, C, H, W), device="cuda", generator=g)
                for sel in SELECTIONS:
                    if sel[0] >= Tn:
                        continue
                    for name, norm in _specs(C):
                        want = tm.statement64(y_hat, y, *sel, **norm)
                        what = (plane, Bn, Tn, C, sel, name)
                        _assert_bits(_op(y_hat, y, sel, **norm), want, what)
                        if (H * W) % 4 == 0:
                            _assert_bits(_op(y_hat, y, sel, aligned=True, **norm), want, what + ("aligned",))
                        if len(tm.selected(Tn, *sel)) == 1:
                            assert bool((want[:, :, 2:5] == 0).all()), what


def _rule(ours, own, want, what):
    """max(2e-7, 3 x own) against float64, in both measures -> the larger ratio ours / bound."""
    def errs(a):
        d = a.double() - want
        return float(d.abs().max() / want.abs().max()), float(d.norm() / want.norm())
    o, w = errs(ours), errs(own)
    ratios = [a / max(FLOOR, 3.0 * b) for a, b in zip(o, w)]
    print("%s: rel-max %.3e (own %.3e) rel-L2 %.3e (own %.3e) -> %.3f %.3f of the bound" % (what, o[0], w[0], o[1], w[1], ratios[0], ratios[1]))
    assert o[0] <= max(FLOOR, 3.0 * w[0]) and o[1] <= max(FLOOR, 3.0 * w[1]), (what, o, w)
    return max(ratios)


@pytest.mark.parametrize("family", tm.FAMILIES)
def test_op_against_float64(family):
    """Every map under max(2e-7, 3 x own) against float64 reductions of the same fp32 fields, own = torch's fp32 reductions,
    for T = 64 and 300 on planes 17x16 (B = 2) and 128x128 (B = 1).  `offset` (1e3 + 1e-2 x) is why the sums are shifted by
    the truth's first frame, `drift` (x + 0.05 t) and T = 300 why they are float64.
    Measured worst ratio ours / bound on MI355X over both planes, both T and the seven maps:
    unit 0.219, tiny 0.200, huge 0.241, offset 0.193, drift 0.284."""
    teg._need_gpu()
    g = torch.Generator(device="cuda").manual_seed(5)
    worst = 0.0
    for Bn, plane in ((2, (17, 16)), (1, (128, 128))):
        for Tn in (64, 300):
            y_hat, y = tm.family(family, (Bn, Tn, 2) + plane, g, device="cuda")
            ours = _op(y_hat, y, aligned=True)
            own, want = tm.own32(y_hat, y), tm.direct64(y_hat, y)
            for k, name in enumerate(tm.NAMES):
                worst = max(worst, _rule(ours[:, :, k], own[:, :, k], want[:, :, k], "%s %dx%d T=%d %s" % ((family,) + plane + (Tn, name))))
    print("%s: worst ratio ours / bound = %.3f" % (family, worst))


def test_op_semantics():
    teg._need_gpu()
    from lns_amd import metrics
    g = torch.Generator(device="cuda").manual_seed(9)
    y = torch.randn((2, 6, 3, 23, 29), device="cuda", generator=g)
    y_hat = y + 0.3 * torch.randn(y.shape, device="cuda", generator=g)
    col = {n: i for i, n in enumerate(tm.NAMES)}
    norm = dict(mean=0.37, std=1.9)
    # P == Q: no error, and the moments of both with equal bits
    s = _op(y, y, **norm)
    assert bool((s[:, :, col["mse"]] == 0).all()) and bool((s[:, :, col["max_err"]] == 0).all())
    for k in ("var_Q", "cov"):
        assert _same(s[:, :, col["var_P"]].contiguous(), s[:, :, col[k]].contiguous()), k
    assert _same(s[:, :, col["mean_P"]].contiguous(), s[:, :, col["mean_Q"]].contiguous())
    assert bool(((metrics.temporal_correlation(s) - 1).abs() <= 4e-7).all())
    # a truth pixel constant in time: its variance and covariance are exactly 0 (the shift is its value)
    b = y.clone()
    b[1, :, 2, 11, 13] = 0.8125
    s = _op(y_hat, b, **norm)
    assert s[1, 2, col["var_Q"], 11, 13] == 0 and s[1, 2, col["cov"], 11, 13] == 0 and s[1, 2, col["var_P"], 11, 13] > 0
    assert metrics.temporal_correlation(s)[1, 2, 11, 13] == 0
    assert bool((s[:, :, col["var_Q"]] > 0).sum() == s[:, :, col["var_Q"]].numel() - 1)
    assert _same(metrics.rmse_map(s), s[:, :, col["mse"]].sqrt())
    # a NaN in one pixel at one step stays in that pixel of that (b, c): means and mse NaN, the largest error skips it
    clean = _op(y_hat, y, **norm)
    a = y_hat.clone()
    a[1, 3, 2, 11, 13] = float("nan")
    s = _op(a, y, **norm)
    for n in ("mean_P", "mse", "cov"):
        assert bool(torch.isnan(s[1, 2, col[n], 11, 13])), n
    assert s[1, 2, col["var_P"], 11, 13] == 0                       # (v > 0 ? v : 0 of a NaN)
    for n in ("mean_Q", "var_Q", "max_err"):
        assert bool(torch.isfinite(s[1, 2, col[n], 11, 13])), n
    want = tm.statement64(a, y, **norm)
    assert torch.equal(torch.isnan(s), torch.isnan(want)) and int(torch.isnan(s).sum()) == 3
    assert _same(torch.nan_to_num(s), torch.nan_to_num(want))
    keep = torch.ones(s.shape, dtype=torch.bool, device="cuda")
    keep[1, 2, :, 11, 13] = False
    assert torch.equal(s[keep].view(torch.int32), clean[keep].view(torch.int32))
    for n in ("mean_Q", "var_Q"):
        assert s[1, 2, col[n], 11, 13] == clean[1, 2, col[n], 11, 13]


# ---- the streaming calls ------------------------------------------------------------------------------------------------
def _hist_of(args):
    if args.family.startswith("twophase"):
        return (32, [-1.0, -1.0, -300.0, 0.0], [1.0, 1.0, 900.0, 1.0])
    return (64, -6.0, 6.5)


def _check_against_stats_call(r, ref, keep_ref, what):
    assert _same(r.frame, ref.frame) and _same(r.seq, ref.seq), what
    assert _same(r.frames, keep_ref) and _same(r.frames, ref.frames), what
    assert list(r.stats_steps) == list(ref.stats_steps) and _same(r.stats, ref.stats) and torch.equal(r.hist, ref.hist), what
    assert list(r.spectrum_steps) == list(ref.spectrum_steps) and _same(r.spectra, ref.spectra), what


@pytest.mark.parametrize("case", ["ns2d_mini", "twophase_cond"])
def test_streaming_maps_same_bits_as_the_op_on_the_stored_rollout(case):
    """decode_group 1, 2, 3 and the default, one to four decode streams, overlap on and off, the diagnostics mode; the
    conditional preset runs with `param`.  With T = 5 a group holds 1 .. 5 steps, so some groups select nothing."""
    teg._need_gpu()
    from lns_amd import engine
    args, model, eng, xd, yd, pd, norm, denorm, y = teg._setup(case)
    out, f_ref, s_ref = teg._two_call(eng, xd, yd, pd, norm)
    hist = _hist_of(args)
    C = args.in_channels
    stats_steps, spectrum_steps = (0, 4), (3,)
    ref = eng.rollout_eval_stats(xd, yd, param=pd, keep_steps=KEEP, stats_steps=stats_steps, hist=hist, spectrum_steps=spectrum_steps, **norm)
    keep_ref = out[:, list(KEEP)].contiguous()
    assert _same(ref.frame, f_ref) and _same(ref.seq, s_ref)
    want = {sel: eng.time_maps(out, yd, map_steps=sel, **norm) for sel in SELECTIONS}
    torch.cuda.synchronize()
    for sel in SELECTIONS:
        _assert_bits(want[sel], tm.statement64(out, yd, *sel, **norm), (case, sel, "op"))
    try:
        i = 0
        for dg in (1, 2, 3, 0):
            for ds, ov in ((1, 1), (2, 1), (3, 1), (4, 1), (3, 0)):
                eng.set_option("decode_group", dg)
                eng.set_option("decode_streams", ds)
                eng.set_option("overlap", ov)
                sels = SELECTIONS if (ds, ov) == (3, 1) else (SELECTIONS[i % 3],)
                i += 1
                for sel in sels:
                    r = eng.rollout_eval_maps(xd, yd, param=pd, keep_steps=KEEP, map_steps=sel, stats_steps=stats_steps, hist=hist,
                                              spectrum_steps=spectrum_steps, **norm)
                    torch.cuda.synchronize()
                    what = (case, dg, ds, ov, sel)
                    assert isinstance(r, engine.EvalMaps) and r.map_steps == sel and r.maps.shape == (B, C, 7, args.Ly, args.Lx)
                    _assert_bits(r.maps, want[sel], what)
                    _check_against_stats_call(r, ref, keep_ref, what)
                    eng.check_finite(B, xd.device)
        eng.set_option("decode_group", 2)
        eng.set_option("decode_streams", 3)
        eng.set_option("overlap", 1)
        eng.timing_enable(True)                                    # diagnostics mode: everything on the caller's stream
        r = eng.rollout_eval_maps(xd, yd, param=pd, keep_steps=KEEP, map_steps=(1, 2), stats_steps=stats_steps, hist=hist,
                                  spectrum_steps=spectrum_steps, **norm)
        torch.cuda.synchronize()
        eng.timing_enable(False)
        _assert_bits(r.maps, want[(1, 2)], (case, "timing"))
        _check_against_stats_call(r, ref, keep_ref, (case, "timing"))
        # maps alone: no statistics, no spectra, no kept frames
        r = eng.rollout_eval_maps(xd, yd, param=pd, map_steps=slice(1, None, 2), **norm)
        torch.cuda.synchronize()
        _assert_bits(r.maps, want[(1, 2)], (case, "alone"))
        assert r.stats is None and r.hist is None and r.spectra is None and r.frames is None
        assert list(r.stats_steps) == [] and list(r.spectrum_steps) == [] and _same(r.frame, f_ref) and _same(r.seq, s_ref)
        # the drop-in entry
        extra = (pd,) if pd is not None else ()
        v = model.validate_maps(xd, yd, *extra, map_steps=(3, 4), stats_steps=stats_steps, hist=hist, spectrum_steps=spectrum_steps,
                                keep_steps=KEEP, **norm)
        torch.cuda.synchronize()
        _assert_bits(v.maps, want[(3, 4)], (case, "validate_maps"))
        _check_against_stats_call(v, ref, keep_ref, (case, "validate_maps"))
        with pytest.raises(TypeError):
            model.validate_maps(xd, yd, *extra, 1.0, **norm)
    finally:
        eng.timing_enable(False)
        eng.set_option("decode_group", 1)
        eng.set_option("decode_streams", 3)
        eng.set_option("overlap", 1)


def _chunked_with_every_selection(case):
    """Chunks 4 + 3 of a horizon of 7 at B = 2 under decode_group = 2 (the second chunk ends in a ragged group), each carrying
    spectra, statistics with histograms, maps and kept frames together: the two chunks against the one call, bit for bit, and
    the maps against the op on the stored rollout."""
    args, model, eng, xd, yd, pd, norm, denorm, y = teg._setup(case)
    C, T7, x2 = args.in_channels, 7, xd[:2].contiguous()
    g = torch.Generator(device="cuda").manual_seed(78)
    y7 = torch.randn((2, T7, C, args.Ly, args.Lx), device="cuda", generator=g)
    sel = dict(map_steps=(1, 2), hist=_hist_of(args))
    z0 = eng.encode(x2)
    try:
        eng.set_option("decode_group", 2)
        one = eng.rollout_eval_maps(x2, y7, keep_steps=(1, 4, 6), stats_steps=(1, 2, 6), spectrum_steps=(0, 3, 6), **sel, **norm)
        a = eng.rollout_latent_eval_maps(z0, y7, steps=4, t0=0, keep_steps=(1,), stats_steps=(1, 2), spectrum_steps=(0, 3), **sel,
                                         **norm)
        b = eng.rollout_latent_eval_maps(a.z_last, y7, steps=3, t0=4, keep_steps=(0, 2), stats_steps=(2,), spectrum_steps=(2,),
                                         frame=a.frame, seq=a.seq, maps=a.maps, **sel, **norm)
        torch.cuda.synchronize()
    finally:
        eng.set_option("decode_group", 1)
    _assert_bits(one.maps, eng.time_maps(eng.rollout(x2, T7), y7, map_steps=(1, 2), **norm), (case, "one call"))
    assert b.maps is a.maps and b.frame is a.frame and b.seq is a.seq
    _assert_bits(b.maps, one.maps, (case, "chunked"))
    assert _same(b.frame, one.frame) and _same(b.seq, one.seq)
    assert _same(torch.cat([a.stats, b.stats], 1), one.stats) and torch.equal(torch.cat([a.hist, b.hist], 1), one.hist)
    assert _same(torch.cat([a.spectra, b.spectra], 1), one.spectra)
    assert _same(torch.cat([a.frames, b.frames], 1), one.frames)


@pytest.mark.parametrize("case", ["ns2d_mini", "twophase_cond", "ns2d_mini-4+3-every-selection"])
def test_chunked_latent_calls_reproduce_the_one_call_result(case):
    """Chunks 3 + 1 + 4 of a horizon of 8 on one workspace.  (3, 2): map_from lies in the second chunk; (4, 3): the first two
    chunks select nothing.  maps is untouched until the chunk that completes the horizon.  The third case:
    _chunked_with_every_selection."""
    teg._need_gpu()
    if case.endswith("-every-selection"):
        return _chunked_with_every_selection(case.split("-")[0])
    args, model, eng, xd, yd, pd, norm, denorm, y = teg._setup(case)
    C, T8 = args.in_channels, 8
    g = torch.Generator(device="cuda").manual_seed(77)
    y8 = torch.randn((B, T8, C, args.Ly, args.Lx), device="cuda", generator=g)
    out = eng.rollout(xd, T8, param=pd)
    z0 = eng.encode(xd) if not eng.cfg.cond_encoder else eng.encode(xd, pd)
    for sel in ((0, 1), (3, 2), (4, 3)):
        one = eng.rollout_eval_maps(xd, y8, param=pd, keep_steps=(0, 3, 7), map_steps=sel, stats_steps=None, spectrum_steps=(3, 5), **norm)
        torch.cuda.synchronize()
        _assert_bits(one.maps, eng.time_maps(out, y8, map_steps=sel, **norm), (case, sel, "one call"))
        maps = torch.full((B, C, 7, args.Ly, args.Lx), -7.5, device="cuda")
        a = eng.rollout_latent_eval_maps(z0, y8, steps=3, t0=0, param=pd, keep_steps=(0,), map_steps=sel, stats_steps=None,
                                         spectrum_steps=(), maps=maps, **norm)
        torch.cuda.synchronize()
        assert a.maps is maps and bool((maps == -7.5).all()), (case, sel)
        b = eng.rollout_latent_eval_maps(a.z_last, y8, steps=1, t0=3, param=pd, keep_steps=(0,), map_steps=sel, stats_steps=None,
                                         spectrum_steps=(0,), frame=a.frame, seq=a.seq, maps=maps, **norm)
        torch.cuda.synchronize()
        assert bool((maps == -7.5).all()), (case, sel)
        c = eng.rollout_latent_eval_maps(b.z_last, y8, steps=4, t0=4, param=pd, keep_steps=(3,), map_steps=sel, stats_steps=None,
                                         spectrum_steps=(1,), frame=a.frame, seq=a.seq, maps=maps, **norm)
        torch.cuda.synchronize()
        _assert_bits(c.maps, one.maps, (case, sel, "chunked"))
        assert _same(c.frame, one.frame) and _same(c.seq, one.seq)
        assert _same(torch.cat([a.stats, b.stats, c.stats], 1), one.stats)
        assert a.spectra is None and _same(torch.cat([b.spectra, c.spectra], 1), one.spectra)
        assert _same(torch.cat([a.frames, b.frames, c.frames], 1), one.frames)


def test_workspace_is_the_evaluation_workspace_plus_the_state():
    teg._need_gpu()
    from lns_amd import _lib, engine
    args, model, eng, xd, yd, pd, norm, denorm, y = teg._setup("ns2d_mini")
    L, h = eng._L, eng._h
    try:
        eng.set_option("decode_group", 2)
        n1, n2 = ctypes.c_size_t(0), ctypes.c_size_t(0)
        assert L.lns_rollout_eval_workspace_bytes(h, B, ctypes.byref(n1)) == 0
        assert L.lns_rollout_eval_maps_workspace_bytes(h, B, ctypes.byref(n2)) == 0
        C, HW = args.in_channels, args.Ly * args.Lx

        def up(v):
            return (v + 255) // 256 * 256
        assert n2.value == up(n1.value) + up(B * C * HW * 52)         # include/lns.h
        spec = engine.eval_spec(C, **norm)
        frame = torch.empty((B, T, C), dtype=torch.float32, device="cuda")
        seq = torch.empty((B, C), dtype=torch.float32, device="cuda")
        maps = torch.full((B, C, 7, args.Ly, args.Lx), -7.5, device="cuda")
        ws = torch.full((n2.value + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        q = _lib.LnsEvalSelect()
        q.size = ctypes.sizeof(_lib.LnsEvalSelect)
        q.map_from, q.map_every, q.maps_out = 1, 2, maps.data_ptr()

        def run(nbytes):
            return L.lns_rollout_eval_maps(h, xd.data_ptr(), None, yd.data_ptr(), B, T, ctypes.byref(spec), frame.data_ptr(),
                                           seq.data_ptr(), None, 0, None, ws.data_ptr(), nbytes, stream, ctypes.byref(q))
        assert run(n2.value - 1) == _lib.LNS_ENOMEM and "workspace" in L.lns_last_error(h).decode()
        torch.cuda.synchronize()
        assert bool((ws == 0xA5).all()) and bool((maps == -7.5).all())   # refused before any launch
        assert run(n2.value) == 0
        torch.cuda.synchronize()
        assert bool((ws[n2.value:] == 0xA5).all())
        out, f_ref, s_ref = teg._two_call(eng, xd, yd, pd, norm)
        _assert_bits(maps, eng.time_maps(out, yd, map_steps=(1, 2), **norm), "workspace")
        assert _same(frame, f_ref) and _same(seq, s_ref)
    finally:
        eng.set_option("decode_group", 1)

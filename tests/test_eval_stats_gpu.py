"""GPU (-m gpu): field statistics -- correlation, gradient error, moments, extrema and value histograms (include/lns.h
"field statistics").

The op (lns_op_field_stats) against tests/field_stats_reference.py: BIT FOR BIT against `statement32` (the statement as
unfused fp32 torch ops in the written reduction order) and exactly against the numpy bin rule; against float64 under the
project's rule max(2e-7, 3 x own) in both of its measures, every one of the 12 columns gated, `own` being torch's fp32
reductions; against the real reference's recorded float64 values (tests/golden/field_stats.npz) under the same rule.

The streaming calls (lns_rollout_eval_stats, lns_rollout_latent_eval_stats) against the op on the stored rollout, BIT FOR
BIT: one block owns one plane and runs the op's device function, so neither the grouping nor a scheduling option can show;
frame / seq / kept frames are held to lns_rollout_eval's bits and the spectra to lns_rollout_eval_spectrum's in the same call."""
import ctypes
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import field_stats_reference as fr  # noqa: E402
import test_eval_gpu as teg  # noqa: E402
from helpers import ROOT  # noqa: E402

pytestmark = pytest.mark.gpu

B, T, KEEP = teg.B, teg.T, teg.KEEP
PLANES = [(1, 1), (1, 7), (2, 2), (3, 5), (17, 16), (23, 29), (61, 121)]
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


def _guarded(shape, dtype, sentinel):
    """-> (flat buffer, the view of `shape` inside it at an odd element offset, check()) with GUARD + 1 / GUARD sentinels around."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD + 1,), sentinel, dtype=dtype, device="cuda")
    view = buf[GUARD + 1:GUARD + 1 + n].view(shape)

    def check():
        assert bool((buf[:GUARD + 1] == sentinel).all()) and bool((buf[GUARD + 1 + n:] == sentinel).all()), "guard overwritten"
    return buf, view, check


def _op(y_hat, y, hist=None, **norm):
    """lns_op_field_stats through ctypes on unaligned inputs into guarded, unaligned outputs -> (stats, counts or None)."""
    from lns_amd import _lib, engine
    L = _lib.lib()
    Bn, Tn, C, H, W = (int(v) for v in y.shape)
    a, g = _unaligned(y_hat), _unaligned(y)
    spec = engine.eval_spec(C, **norm)
    hs = engine.stats_spec(C, hist)
    _, stats, chk_s = _guarded((Bn, Tn, C, 12), torch.float32, -7.5)
    counts, chk_c = None, None
    if hs is not None:
        _, counts, chk_c = _guarded((Bn, Tn, C, 2, hs.nbins + 2), torch.int32, -77)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.lns_op_field_stats(a.data_ptr(), g.data_ptr(), Bn, Tn, C, H, W, ctypes.byref(spec),
                              ctypes.byref(hs) if hs is not None else None, stats.data_ptr(),
                              counts.data_ptr() if counts is not None else None, stream)
    assert rc == 0, L.lns_create_error().decode()
    torch.cuda.synchronize()
    chk_s()
    if chk_c:
        chk_c()
    return stats.clone(), (counts.clone() if counts is not None else None)


def _specs(C):
    """The scalar spec and a per-channel one with walls on channel 0 and the clamp on the last channel, with histogram edges."""
    scalar = dict(mean=0.37, std=1.9, eps=1e-8)
    per_ch = dict(mean=[0.4, -0.2, 0.5][:C], std=[2.1, 1.7, 0.35][:C], zero_wall_channels=(0,), clamp_channels=(C - 1,),
                  clamp=(0.0, 1.0 + 1e-8))
    return (("scalar", scalar, (7, -2.0, 3.0)),
            ("per_channel", per_ch, (256, [-3.0, -2.5, 0.0][:C], [4.0, 2.0, 1.0][:C])))


@pytest.mark.parametrize("plane", PLANES, ids=lambda p: "%dx%d" % p)
def test_op_has_the_bits_of_the_statement(plane):
    """One term (1x1), no gradient terms (1x7, 2x2), a partial pass (3x5), a tail past 256 (17x16), two full passes plus a
    tail (23x29), 28 passes plus a tail (61x121)."""
    teg._need_gpu()
    H, W = plane
    g = torch.Generator(device="cuda").manual_seed(1000 * H + W)
    for Bn in (1, 3):
        for Tn in (1, 2):
            for C in (1, 3):
                y = torch.randn((Bn, Tn, C, H, W), device="cuda", generator=g)
                y_hat = y + 0.3 * torch.randn((Bn, Tn, C, H, W), device="cuda", generator=g)
                for name, norm, hist in _specs(C):
                    stats, counts = _op(y_hat, y, hist, **norm)
                    want = fr.statement32(y_hat, y, **norm)
                    what = (plane, Bn, Tn, C, name)
                    assert stats.shape == want.shape and stats.dtype == torch.float32
                    diff = (stats.view(torch.int32) != want.view(torch.int32)).nonzero()
                    assert diff.numel() == 0, (what, diff[:4].tolist(), stats[tuple(diff[0])].item(), want[tuple(diff[0])].item())
                    wc = fr.counts(y_hat, y, *hist, **norm)
                    assert np.array_equal(counts.cpu().numpy().astype(np.int64), wc), what
                    assert int(wc.sum()) == 2 * y.numel()
                    # without histograms: the same statistics
                    assert _same(_op(y_hat, y, None, **norm)[0], stats), what
                    if H < 3 or W < 3:
                        assert bool((stats[..., 6:8] == 0).all()), what


def _rule(ours, own, want, what):
    """max(2e-7, 3 x own) against float64, in both measures -> the larger ratio ours / bound (the _rule of test_ensemble_score_gpu)."""
    def errs(a):
        d = a.double() - want
        return float(d.abs().max() / want.abs().max()), float(d.norm() / want.norm())
    o, w = errs(ours), errs(own)
    ratios = [a / max(FLOOR, 3.0 * b) for a, b in zip(o, w)]
    print("%s: rel-max %.3e (own %.3e) rel-L2 %.3e (own %.3e) -> %.3f %.3f of the bound" % (what, o[0], w[0], o[1], w[1], ratios[0], ratios[1]))
    assert o[0] <= max(FLOOR, 3.0 * w[0]) and o[1] <= max(FLOOR, 3.0 * w[1]), (what, o, w)
    return max(ratios)


def _family(name, shape, g):
    x = torch.randn(shape, device="cuda", generator=g)
    q = {"unit": x, "tiny": 1e-12 * x, "huge": 1e12 * x, "offset": 1e3 + 1e-2 * x}[name]
    return q + 0.3 * q.std() * torch.randn(shape, device="cuda", generator=g), q


@pytest.mark.parametrize("family", ["unit", "tiny", "huge", "offset"])
def test_op_against_float64(family):
    """Every column under max(2e-7, 3 x own), own = torch's fp32 reductions of the same fp32 fields.  `offset` (1e3 + 1e-2 x)
    is why the variance is two-pass: one pass loses all of it.  Measured worst ratio ours / bound on MI355X over the four
    planes and twelve columns: unit 0.448, tiny 0.511, huge 0.616, offset 0.463."""
    teg._need_gpu()
    g = torch.Generator(device="cuda").manual_seed(5)
    worst = 0.0
    for plane in ((3, 5), (17, 16), (61, 121), (128, 128)):
        y_hat, y = _family(family, (2, 2, 3) + plane, g)
        ours = _op(y_hat, y)[0]
        own, want = fr.stats32_torch(y_hat, y), fr.stats64(y_hat, y)
        for k, name in enumerate(fr.NAMES):
            worst = max(worst, _rule(ours[..., k], own[..., k], want[..., k], "%s %dx%d %s" % ((family,) + plane + (name,))))
    print("%s: worst ratio ours / bound = %.3f" % (family, worst))


@pytest.mark.parametrize("name", list(fr.GOLDEN))
def test_op_against_the_recorded_reference_values(name):
    teg._need_gpu()
    gold = np.load(os.path.join(ROOT, "tests", "golden", "field_stats.npz"))
    yh, y = (torch.from_numpy(a).cuda() for a in fr.golden_inputs(name))
    norm = fr.golden_norm(name)
    ours = _op(yh, y, **norm)[0]
    own = fr.stats32_torch(yh, y, **norm)
    for k in ("cos", "grad_y", "grad_x"):
        i = fr.NAMES.index(k)
        _rule(ours[..., i], own[..., i], torch.from_numpy(gold["%s_%s" % (name, k)]).cuda(), "%s %s" % (name, k))


def test_op_edge_cases():
    teg._need_gpu()
    g = torch.Generator(device="cuda").manual_seed(9)
    y = torch.randn((2, 2, 3, 23, 29), device="cuda", generator=g)
    y_hat = y + 0.3 * torch.randn(y.shape, device="cuda", generator=g)
    col = {n: i for i, n in enumerate(fr.NAMES)}
    # a constant plane: variance 0 and correlation 0, in the forecast or in the truth
    a, b = y_hat.clone(), y.clone()
    a[0, 1, 2] = 0.0625                                            # -> 0.625: every partial sum and the mean are exact in fp32
    b[1, 0, 0] = -3.0
    s = _op(a, b, mean=0.5, std=2.0)[0]
    assert s[0, 1, 2, col["var_P"]] == 0 and s[0, 1, 2, col["corr"]] == 0 and s[0, 1, 2, col["var_Q"]] > 0
    assert s[1, 0, 0, col["var_Q"]] == 0 and s[1, 0, 0, col["corr"]] == 0
    assert s[0, 1, 2, col["min_P"]] == s[0, 1, 2, col["max_P"]] == s[0, 1, 2, col["mean_P"]]
    assert bool((s[0, 0, :, col["corr"]] > 0.9).all())
    # P == Q: correlation 1 to rounding, gradient error exactly 0, equal moments and extrema
    s = _op(y, y, mean=0.37, std=1.9)[0]
    assert bool(((s[..., col["corr"]] - 1).abs() <= 4e-7).all()) and bool(((s[..., col["cos"]] - 1).abs() <= 4e-7).all())
    assert bool((s[..., col["grad_y"]] == 0).all()) and bool((s[..., col["grad_x"]] == 0).all())
    for p, q in (("mean_P", "mean_Q"), ("var_P", "var_Q"), ("min_P", "min_Q"), ("max_P", "max_Q")):
        assert torch.equal(s[..., col[p]], s[..., col[q]])
    # a NaN pixel stays in its own plane: its sums are NaN, its extrema finite, its counts short by one
    hist = (16, -4.0, 4.0)
    clean, ccounts = _op(y_hat, y, hist)
    a = y_hat.clone()
    a[1, 0, 2, 11, 13] = float("nan")
    s, c = _op(a, y, hist)
    for n in ("mean_P", "cos", "grad_y", "grad_x"):
        assert bool(torch.isnan(s[1, 0, 2, col[n]])), n
    for n in ("min_P", "max_P", "mean_Q", "var_Q", "min_Q", "max_Q"):
        assert bool(torch.isfinite(s[1, 0, 2, col[n]])), n
    assert _same(s[1, 0, 2, 8:], fr.statement32(a, y)[1, 0, 2, 8:])
    assert int(c[1, 0, 2, 0].sum()) == 23 * 29 - 1 and int(c[1, 0, 2, 1].sum()) == 23 * 29
    keep = torch.ones(s.shape[:3], dtype=torch.bool, device="cuda")
    keep[1, 0, 2] = False
    assert torch.equal(s[keep].view(torch.int32), clean[keep].view(torch.int32)) and torch.equal(c[keep], ccounts[keep])
    assert torch.equal(c[1, 0, 2, 1], ccounts[1, 0, 2, 1])


def test_op_refused_arguments():
    teg._need_gpu()
    from lns_amd import _lib, engine, metrics
    L = _lib.lib()
    y = torch.zeros((1, 1, 2, 4, 4), device="cuda")
    out = torch.zeros((1, 1, 2, 12), device="cuda")
    cnt = torch.zeros((1, 1, 2, 2, 6), dtype=torch.int32, device="cuda")
    spec = engine.eval_spec(2)
    hs = engine.stats_spec(2, (4, 0.0, 1.0))

    def run(a=y, g=y, dims=(1, 1, 2, 4, 4), sp=spec, h=hs, o=out, c=cnt):
        rc = L.lns_op_field_stats(a.data_ptr() if a is not None else None, g.data_ptr() if g is not None else None, *dims,
                                  ctypes.byref(sp) if sp is not None else None, ctypes.byref(h) if h is not None else None,
                                  o.data_ptr() if o is not None else None, c.data_ptr() if c is not None else None, None)
        return rc, L.lns_create_error().decode()
    assert run()[0] == 0
    assert run(c=None)[0] == 0 and run(h=None, c=None)[0] == 0
    for kw, text in ((dict(a=None), "null"), (dict(g=None), "null"), (dict(o=None), "null"), (dict(sp=None), "spec is null"),
                     (dict(dims=(1, 0, 2, 4, 4)), "B, T, C, H, W >= 1"), (dict(dims=(1, 1, 2, 4, 0)), "B, T, C, H, W >= 1"),
                     (dict(h=None), "hist_out needs"), (dict(h=engine.stats_spec(2, (0, 0.0, 1.0))), "nbins"),
                     (dict(h=engine.stats_spec(2, (257, 0.0, 1.0))), "nbins"), (dict(h=engine.stats_spec(2, (4, 1.0, 1.0))), "edges"),
                     (dict(h=engine.stats_spec(2, (4, 0.0, [1.0, float("inf")]))), "edges")):
        rc, msg = run(**kw)
        assert rc == _lib.LNS_EINVAL and text in msg, (kw, rc, msg)
    bad = engine.stats_spec(2, (4, 0.0, 1.0))
    bad.size = 8
    rc, msg = run(h=bad)
    assert rc == _lib.LNS_EINVAL and "size" in msg
    wide = torch.zeros((1, 1, 9, 4, 4), device="cuda")
    assert run(a=wide, g=wide, dims=(1, 1, 9, 4, 4), o=torch.zeros((1, 1, 9, 12), device="cuda"), h=None, c=None)[0] == 0
    rc, msg = run(a=wide, g=wide, dims=(1, 1, 9, 4, 4), o=torch.zeros((1, 1, 9, 12), device="cuda"), h=engine.stats_spec(8, (4, 0.0, 1.0)),
                  c=torch.zeros((1, 1, 9, 2, 6), dtype=torch.int32, device="cuda"))
    assert rc == _lib.LNS_EINVAL and "in_channels <= 8" in msg
    with pytest.raises(_lib.LnsError, match="no CPU fallback"):
        metrics.field_stats(y.cpu(), y.cpu())
    with pytest.raises(_lib.LnsError, match="shape"):
        metrics.field_stats(y, y[:, :, :1])


# ---- the streaming calls ------------------------------------------------------------------------------------------------
def _hist_of(args):
    """Histogram description in the family's denormalised units: scalar edges, or per-channel ones for two-phase."""
    if args.family.startswith("twophase"):
        return (32, [-1.0, -1.0, -300.0, 0.0], [1.0, 1.0, 900.0, 1.0])
    return (64, -6.0, 6.5)


def _reference(eng, out, yd, steps, hist, norm):
    idx = list(range(T)) if steps is None else list(steps)
    stats, counts = eng.field_stats(out[:, idx].contiguous(), yd[:, idx].contiguous(), hist=hist, **norm)
    torch.cuda.synchronize()
    return idx, stats, counts


@pytest.mark.parametrize("case", ["ns2d_mini", "twophase_cond"])
def test_streaming_stats_same_bits_as_the_op_on_the_stored_rollout(case):
    teg._need_gpu()
    args, model, eng, xd, yd, pd, norm, denorm, y = teg._setup(case)
    out, f_ref, s_ref = teg._two_call(eng, xd, yd, pd, norm)
    hist = _hist_of(args)
    C = args.in_channels
    for steps in ((0, 3, 4), None, (2,)):
        idx, ref, cref = _reference(eng, out, yd, steps, hist, norm)
        assert int(cref.sum()) == 2 * B * len(idx) * C * args.Ly * args.Lx
        for keep, spectrum_steps in ((KEEP, ()), ((), (1, 3)), (KEEP, None)):
            r = eng.rollout_eval_stats(xd, yd, param=pd, keep_steps=keep, stats_steps=steps, hist=hist,
                                       spectrum_steps=spectrum_steps, **norm)
            torch.cuda.synchronize()
            what = (case, steps, keep, spectrum_steps)
            assert r.stats.shape == (B, len(idx), C, 12) and list(r.stats_steps) == idx
            assert _same(r.stats, ref) and torch.equal(r.hist, cref), what
            assert _same(r.frame, f_ref) and _same(r.seq, s_ref), what
            if keep:
                assert _same(r.frames, out[:, list(keep)].contiguous()), what
            else:
                assert r.frames is None
            if spectrum_steps == ():
                assert r.spectra is None and list(r.spectrum_steps) == []
            else:
                sp = eng.rollout_eval_spectrum(xd, yd, param=pd, spectrum_steps=spectrum_steps, **norm)
                torch.cuda.synchronize()
                assert list(r.spectrum_steps) == list(sp.spectrum_steps) and _same(r.spectra, sp.spectra), what
            eng.check_finite(B, xd.device)
        # without histograms: the same statistics, no counts
        r = eng.rollout_eval_stats(xd, yd, param=pd, stats_steps=steps, **norm)
        torch.cuda.synchronize()
        assert r.hist is None and _same(r.stats, ref)
    # the statistics are what the statement and float64 say of the same stored fields
    _, ref, cref = _reference(eng, out, yd, None, hist, norm)
    assert _same(ref, fr.statement32(out, yd, **norm))
    assert np.array_equal(cref.cpu().numpy().astype(np.int64), fr.counts(out, yd, *hist, **norm))
    own, want = fr.stats32_torch(out, yd, **norm), fr.stats64(out, yd, **norm)
    planes = torch.ones((B, T, C), dtype=torch.bool, device="cuda")
    planes[0, 0, 0] = False                                        # (the truth plane that denormalises to ~0: an eps-clamp case)
    for k, name in enumerate(fr.NAMES):
        _rule(ref[..., k][planes], own[..., k][planes], want[..., k][planes], "%s %s" % (case, name))


def test_streaming_stats_do_not_depend_on_scheduling_options():
    teg._need_gpu()
    args, model, eng, xd, yd, pd, norm, denorm, y = teg._setup("ns2d_mini")
    out, f_ref, s_ref = teg._two_call(eng, xd, yd, pd, norm)
    hist = _hist_of(args)
    steps, spectrum_steps = (0, 4), (3,)                           # groups of 1, 2, 3 steps: some select nothing
    _, ref, cref = _reference(eng, out, yd, steps, hist, norm)
    sp_ref = eng.energy_spectrum(out[:, list(spectrum_steps)].contiguous(), yd[:, list(spectrum_steps)].contiguous(), **norm)
    keep_ref = out[:, list(KEEP)].contiguous()

    def check(tag):
        r = eng.rollout_eval_stats(xd, yd, param=pd, keep_steps=KEEP, stats_steps=steps, hist=hist, spectrum_steps=spectrum_steps, **norm)
        torch.cuda.synchronize()
        assert _same(r.stats, ref) and torch.equal(r.hist, cref) and _same(r.spectra, sp_ref), tag
        assert _same(r.frame, f_ref) and _same(r.seq, s_ref) and _same(r.frames, keep_ref), tag
    for dg in (1, 2, 3, 0):
        for ds in (1, 3):
            for ov in (0, 1):
                eng.set_option("decode_group", dg)
                eng.set_option("decode_streams", ds)
                eng.set_option("overlap", ov)
                check((dg, ds, ov))
    eng.set_option("decode_group", 2)
    eng.timing_enable(True)                                        # diagnostics mode: everything on the caller's stream
    check("timing")
    eng.timing_enable(False)


@pytest.mark.parametrize("case", ["ns2d_mini", "twophase_cond"])
def test_chunked_latent_calls_reproduce_the_one_call_result(case):
    teg._need_gpu()
    args, model, eng, xd, yd, pd, norm, denorm, y = teg._setup(case)
    hist = _hist_of(args)
    one = eng.rollout_eval_stats(xd, yd, param=pd, keep_steps=KEEP, hist=hist, spectrum_steps=None, **norm)
    torch.cuda.synchronize()
    z0 = eng.encode(xd) if not eng.cfg.cond_encoder else eng.encode(xd, pd)
    a = eng.rollout_latent_eval_stats(z0, yd, steps=3, t0=0, param=pd, keep_steps=(0,), stats_steps=(0, 1, 2), hist=hist,
                                      spectrum_steps=None, **norm)
    b = eng.rollout_latent_eval_stats(a.z_last, yd, steps=2, t0=3, param=pd, keep_steps=(0, 1), stats_steps=None, hist=hist,
                                      spectrum_steps=None, frame=a.frame, seq=a.seq, **norm)
    torch.cuda.synchronize()
    assert _same(torch.cat([a.stats, b.stats], 1), one.stats) and torch.equal(torch.cat([a.hist, b.hist], 1), one.hist), case
    assert _same(torch.cat([a.spectra, b.spectra], 1), one.spectra)
    assert _same(b.frame, one.frame) and _same(b.seq, one.seq)
    assert _same(torch.cat([a.frames, b.frames], 1), one.frames)
    # a selection inside the chunk is relative to the chunk
    c = eng.rollout_latent_eval_stats(a.z_last, yd, steps=2, t0=3, param=pd, stats_steps=(1,), frame=a.frame, seq=a.seq, **norm)
    torch.cuda.synchronize()
    assert _same(c.stats, one.stats[:, 4:5].contiguous()) and c.hist is None and c.spectra is None


def test_workspace_is_the_evaluation_workspace():
    teg._need_gpu()
    from lns_amd import _lib, engine
    args, model, eng, xd, yd, pd, norm, denorm, y = teg._setup("ns2d_mini")
    L, h = eng._L, eng._h
    kdec, ndec, max_steps = 2, 3, 64
    eng.set_option("decode_group", kdec)
    eng.set_option("decode_streams", ndec)
    eng.set_option("eval_max_steps", max_steps)
    n0, n1 = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert L.lns_prepare(h, B, ctypes.byref(n0)) == 0
    assert L.lns_rollout_eval_workspace_bytes(h, B, ctypes.byref(n1)) == 0

    def up(v):
        return (v + 255) // 256 * 256
    C, HW = args.in_channels, args.Ly * args.Lx
    assert n1.value - up(n0.value) == ndec * up(kdec * B * C * HW * 4) + up(B * max_steps * C * 2 * 4)      # include/lns.h, unchanged
    spec = engine.eval_spec(C, **norm)
    hist = _hist_of(args)
    hs = engine.stats_spec(C, hist)
    frame = torch.empty((B, T, C), dtype=torch.float32, device="cuda")
    seq = torch.empty((B, C), dtype=torch.float32, device="cuda")
    stats = torch.empty((B, T, C, 12), dtype=torch.float32, device="cuda")
    counts = torch.empty((B, T, C, 2, hs.nbins + 2), dtype=torch.int32, device="cuda")
    ws = torch.empty(n1.value, dtype=torch.uint8, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    sel = (ctypes.c_int * T)(*range(T))

    def run(nbytes):
        return L.lns_rollout_eval_stats(h, xd.data_ptr(), None, yd.data_ptr(), B, T, ctypes.byref(spec), frame.data_ptr(),
                                        seq.data_ptr(), None, 0, None, ws.data_ptr(), nbytes, stream, None, 0, None,
                                        sel, T, ctypes.byref(hs), stats.data_ptr(), counts.data_ptr())
    assert run(n1.value - 1) == _lib.LNS_ENOMEM and "workspace" in L.lns_last_error(h).decode()
    assert run(n1.value) == 0
    torch.cuda.synchronize()
    out, f_ref, s_ref = teg._two_call(eng, xd, yd, pd, norm)
    _, ref, cref = _reference(eng, out, yd, None, hist, norm)
    assert _same(stats, ref) and torch.equal(counts, cref) and _same(frame, f_ref) and _same(seq, s_ref)


@pytest.mark.parametrize("case", ["ns2d_mini", "twophase_cond"])
def test_validate_stats_is_the_hand_written_composition(case):
    teg._need_gpu()
    from lns_amd import engine, metrics
    args, model, eng, xd, yd, pd, norm, denorm, y = teg._setup(case)
    out, f_ref, s_ref = teg._two_call(eng, xd, yd, pd, norm)
    hist = _hist_of(args)
    extra = (pd,) if pd is not None else ()
    v = model.validate_stats(xd, yd, *extra, stats_steps=slice(None, None, 2), hist=hist, spectrum_steps=(1, 4), keep_steps=KEEP, **norm)
    torch.cuda.synchronize()
    assert isinstance(v, engine.EvalStats) and list(v.stats_steps) == [0, 2, 4] and list(v.spectrum_steps) == [1, 4]
    stats, counts = metrics.field_stats(out[:, [0, 2, 4]].contiguous(), yd[:, [0, 2, 4]].contiguous(), hist=hist, **norm)
    assert _same(v.stats, stats) and torch.equal(v.hist, counts)
    assert _same(v.spectra, metrics.energy_spectrum(out[:, [1, 4]].contiguous(), yd[:, [1, 4]].contiguous(), **norm))
    assert _same(v.frame, f_ref) and _same(v.seq, s_ref) and _same(v.frames, out[:, list(KEEP)].contiguous())
    # the defaults: every step, no histograms, no spectra, no kept frames
    d = model.validate_stats(xd, yd, *extra, **norm)
    torch.cuda.synchronize()
    assert list(d.stats_steps) == list(range(T)) and d.hist is None and d.spectra is None and d.frames is None
    assert _same(d.stats, metrics.field_stats(out, yd, **norm)[0])
    t = metrics.correlation_time(d.stats[..., metrics.FIELD_STATS.index("corr")], d.stats_steps, threshold=0.8)
    assert t.shape == (B, args.in_channels) and t.dtype == torch.int64
    with pytest.raises(TypeError):
        model.validate_stats(xd, yd, *extra, 1.0, **norm)

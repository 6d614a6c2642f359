"""GPU (-m gpu): flow diagnostics -- vorticity, divergence, kinetic energy, enstrophy (include/lns.h "flow diagnostics").

The ops (lns_op_flow_stats, lns_op_vorticity) against tests/flow_stats_reference.py: BIT FOR BIT against `statement32` /
`vorticity32` (the statement as unfused fp32 torch ops in the written order) and exactly against the numpy bin rule; against
float64 under the project's rule max(2e-7, 3 x own) in both of its measures, every one of the 12 columns gated, `own` being
torch's fp32 reductions.

The streaming calls (lns_rollout_eval_flow, lns_rollout_latent_eval_flow) against the ops on the stored rollout, BIT FOR BIT:
one block owns one frame and runs the op's device function, so neither the grouping nor a scheduling option nor the chunking
can show; frame / seq / kept frames are held to lns_rollout_eval's bits, statistics and spectra to their own calls'."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import flow_stats_reference as fl  # noqa: E402
import test_eval_gpu as teg  # noqa: E402
import test_eval_stats_gpu as tes  # noqa: E402

pytestmark = pytest.mark.gpu

B, T, KEEP = teg.B, teg.T, teg.KEEP
PLANES = tes.PLANES                                   # 1x1, 1x7, 2x2, 3x5, 17x16, 23x29, 61x121
BOUNDARIES = ((fl.WALL, fl.PERIODIC), (fl.PERIODIC, fl.PERIODIC), (fl.WALL, fl.WALL))
DX, DY = 0.3, 0.7                                     # neither 1 / d nor 1 / (2 d) is a power of two: the products round
_same, _unaligned, _guarded, _rule = teg._same, tes._unaligned, tes._guarded, tes._rule


def _fspec(u, v, bc, hist=None, dx=DX, dy=DY):
    from lns_amd import engine, metrics
    return engine.flow_spec(u, v, dx, dy, tuple(metrics.FLOW_BOUNDARIES[b] for b in bc), hist)


def _op(y_hat, y, u, v, bc, hist=None, dx=DX, dy=DY, **norm):
    """lns_op_flow_stats through ctypes on unaligned inputs into guarded, unaligned outputs -> (flow, counts or None)."""
    from lns_amd import _lib, engine
    L = _lib.lib()
    Bn, Tn, C, H, W = (int(n) for n in y.shape)
    a, g = _unaligned(y_hat), _unaligned(y)
    spec, fs = engine.eval_spec(C, **norm), _fspec(u, v, bc, hist, dx, dy)
    _, flow, chk_f = _guarded((Bn, Tn, 12), torch.float32, -7.5)
    counts, chk_c = None, None
    if hist is not None:
        _, counts, chk_c = _guarded((Bn, Tn, 2, fs.nbins + 2), torch.int32, -77)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.lns_op_flow_stats(a.data_ptr(), g.data_ptr(), Bn, Tn, C, H, W, ctypes.byref(spec), ctypes.byref(fs), flow.data_ptr(),
                             counts.data_ptr() if counts is not None else None, stream)
    assert rc == 0, L.lns_create_error().decode()
    torch.cuda.synchronize()
    chk_f()
    if chk_c:
        chk_c()
    return flow.clone(), (counts.clone() if counts is not None else None)


def _op_vorticity(x, u, v, bc, dx=DX, dy=DY, **norm):
    """lns_op_vorticity through ctypes on an unaligned input into a guarded, unaligned output."""
    from lns_amd import _lib, engine
    L = _lib.lib()
    Bn, Tn, C, H, W = (int(n) for n in x.shape)
    a = _unaligned(x)
    spec, fs = engine.eval_spec(C, **norm), _fspec(u, v, bc, None, dx, dy)
    _, out, chk = _guarded((Bn, Tn, H, W), torch.float32, -7.5)
    rc = L.lns_op_vorticity(a.data_ptr(), Bn, Tn, C, H, W, ctypes.byref(spec), ctypes.byref(fs), out.data_ptr(),
                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.lns_create_error().decode()
    torch.cuda.synchronize()
    chk()
    return out.clone()


def _specs(C, u, v):
    """The scalar spec and a per-channel one with walls on the velocity channels and the clamp on the last channel."""
    scalar = dict(mean=0.37, std=1.9, eps=1e-8)
    per_ch = dict(mean=[0.4, -0.2, 0.5, 0.1][:C], std=[2.1, 1.7, 0.35, 1.3][:C], zero_wall_channels=(u, v), clamp_channels=(C - 1,),
                  clamp=(-1.5, 1.0 + 1e-8))
    return (("scalar", scalar, (7, -9.0, 11.0)), ("per_channel", per_ch, (256, -12.5, 12.0)))


@pytest.mark.parametrize("plane", PLANES, ids=lambda p: "%dx%d" % p)
def test_ops_have_the_bits_of_the_statement(plane):
    """One term (1x1), axes of length 1 and 2 (1x7, 2x2), a partial pass (3x5), a tail past 256 (17x16), two full passes plus
    a tail (23x29), 28 passes plus a tail (61x121); every boundary pair, both kinds of spec, both channel pairs."""
    teg._need_gpu()
    H, W = plane
    g = torch.Generator(device="cuda").manual_seed(1000 * H + W)
    for Bn in (1, 3):
        for Tn in (1, 2):
            for C, (u, v) in ((2, (0, 1)), (4, (2, 0))):
                y = torch.randn((Bn, Tn, C, H, W), device="cuda", generator=g)
                y_hat = y + 0.3 * torch.randn((Bn, Tn, C, H, W), device="cuda", generator=g)
                for name, norm, hist in _specs(C, u, v):
                    for bc in BOUNDARIES:
                        what = (plane, Bn, Tn, C, name, bc)
                        kw = dict(u=u, v=v, dx=DX, dy=DY, bc=bc, **norm)
                        flow, counts = _op(y_hat, y, u, v, bc, hist, **norm)
                        want = fl.statement32(y_hat, y, **kw)
                        assert flow.shape == want.shape and flow.dtype == torch.float32
                        diff = (flow.view(torch.int32) != want.view(torch.int32)).nonzero()
                        assert diff.numel() == 0, (what, diff[:4].tolist(), flow[tuple(diff[0])].item(), want[tuple(diff[0])].item())
                        wc = fl.counts(y_hat, y, *hist, **kw)
                        assert np.array_equal(counts.cpu().numpy().astype(np.int64), wc), what
                        assert int(wc.sum()) == 2 * Bn * Tn * H * W
                        assert _same(_op(y_hat, y, u, v, bc, None, **norm)[0], flow), what      # without the histogram: the same
                        for x in (y_hat, y):
                            assert _same(_op_vorticity(x, u, v, bc, **norm), fl.vorticity32(x, **kw)), what
                        if H == 1 and W == 1:
                            assert bool((flow[..., 2:8] == 0).all()) and bool((flow[..., 9:] == 0).all()), what


def test_op_against_numpy_gradient_on_walls():
    """The op itself (not only the reference) is numpy.gradient(edge_order=1) / a rolled difference, to fp32 rounding."""
    teg._need_gpu()
    g = torch.Generator(device="cuda").manual_seed(17)
    x = torch.randn((1, 1, 2, 23, 29), device="cuda", generator=g)
    a = x[0, 0].double().cpu().numpy()
    for bc in BOUNDARIES:
        w = _op_vorticity(x, 0, 1, bc, dx=0.25, dy=0.5)[0, 0].double().cpu().numpy()
        dxv = np.gradient(a[1], 0.25, axis=1, edge_order=1) if bc[1] else (np.roll(a[1], -1, 1) - np.roll(a[1], 1, 1)) / 0.5
        dyu = np.gradient(a[0], 0.5, axis=0, edge_order=1) if bc[0] else (np.roll(a[0], -1, 0) - np.roll(a[0], 1, 0)) / 1.0
        assert np.allclose(w, dxv - dyu, rtol=0, atol=4e-6), bc


@pytest.mark.parametrize("family", ["unit", "tiny", "huge", "offset"])
def test_op_against_float64(family):
    """Every column under max(2e-7, 3 x own) in both measures, own = torch's fp32 reductions of the same fp32 fields.
    Measured worst ratio ours / bound on MI355X over the four planes and twelve columns: unit 0.578, tiny 0.584,
    huge 0.624, offset 0.559."""
    teg._need_gpu()
    g = torch.Generator(device="cuda").manual_seed(5)
    bc = (fl.WALL, fl.PERIODIC)
    worst = 0.0
    for plane in ((3, 5), (17, 16), (61, 121), (128, 128)):
        y_hat, y = tes._family(family, (2, 2, 3) + plane, g)
        ours = _op(y_hat, y, 0, 1, bc)[0]
        kw = dict(u=0, v=1, dx=DX, dy=DY, bc=bc)
        own, want = fl.stats32_torch(y_hat, y, **kw), fl.stats64(y_hat, y, **kw)
        for k, name in enumerate(fl.NAMES):
            worst = max(worst, _rule(ours[..., k], own[..., k], want[..., k], "%s %dx%d %s" % ((family,) + plane + (name,))))
    print("%s: worst ratio ours / bound = %.3f" % (family, worst))


def test_op_edge_cases():
    teg._need_gpu()
    g = torch.Generator(device="cuda").manual_seed(9)
    y = torch.randn((2, 2, 3, 23, 29), device="cuda", generator=g)
    y_hat = y + 0.3 * torch.randn(y.shape, device="cuda", generator=g)
    col = {n: i for i, n in enumerate(fl.NAMES)}
    bc = (fl.WALL, fl.PERIODIC)
    # P == Q: no error, cosine 1 to rounding, equal columns
    s = _op(y, y, 0, 1, bc)[0]
    assert bool((s[..., col["vort_err"]] == 0).all()) and bool((s[..., col["vel_err"]] == 0).all())
    assert bool(((s[..., col["vort_cos"]] - 1).abs() <= 4e-7).all())
    for p, q in (("ke_P", "ke_Q"), ("ens_P", "ens_Q"), ("div_P", "div_Q"), ("maxvort_P", "maxvort_Q")):
        assert torch.equal(s[..., col[p]], s[..., col[q]])
    # a uniform flow has no vorticity and no divergence, whatever the boundaries
    flat = torch.full_like(y, 0.625)
    s = _op(flat, y, 0, 1, bc, mean=0.5, std=2.0)[0]
    for n in ("ens_P", "div_P", "maxvort_P", "maxdiv_P"):
        assert bool((s[..., col[n]] == 0).all()), n
    assert bool((s[..., col["ke_P"]] == 0.5 * (2 * 1.75 ** 2)).all())
    # a NaN pixel of a velocity channel stays in its own frame: its sums are NaN, its maxima finite, its counts short
    hist = (16, -20.0, 20.0)
    clean, ccounts = _op(y_hat, y, 0, 1, bc, hist)
    a = y_hat.clone()
    a[1, 0, 1, 11, 13] = float("nan")
    s, c = _op(a, y, 0, 1, bc, hist)
    for n in ("ke_P", "ens_P", "div_P", "vort_err", "vort_cos", "vel_err"):
        assert bool(torch.isnan(s[1, 0, col[n]])), n
    for n in ("ke_Q", "ens_Q", "div_Q", "maxvort_P", "maxvort_Q", "maxdiv_P"):
        assert bool(torch.isfinite(s[1, 0, col[n]])), n
    assert _same(s[1, 0, 9:], fl.statement32(a, y, dx=DX, dy=DY, bc=bc)[1, 0, 9:])
    # (a central difference does not read its own pixel: the NaN of V reaches the vorticity of its two x-neighbours)
    assert int(c[1, 0, 0].sum()) == 23 * 29 - 2 and torch.equal(c[1, 0, 1], ccounts[1, 0, 1])
    keep = torch.ones(s.shape[:2], dtype=torch.bool, device="cuda")
    keep[1, 0] = False
    assert torch.equal(s[keep].view(torch.int32), clean[keep].view(torch.int32)) and torch.equal(c[keep], ccounts[keep])
    # a channel that is not a velocity channel does not enter
    b = y_hat.clone()
    b[:, :, 2] = float("nan")
    assert _same(_op(b, y, 0, 1, bc)[0], _op(y_hat, y, 0, 1, bc)[0])


def test_wrappers_refuse_and_agree_with_the_op():
    teg._need_gpu()
    from lns_amd import _lib, metrics
    g = torch.Generator(device="cuda").manual_seed(2)
    y = torch.randn((2, 2, 3, 17, 16), device="cuda", generator=g)
    y_hat = y + 0.3 * torch.randn(y.shape, device="cuda", generator=g)
    bc = (fl.WALL, fl.PERIODIC)
    flow, counts = metrics.flow_stats(y_hat, y, u=2, v=0, dx=DX, dy=DY, boundary=("wall", "periodic"), vort_hist=(9, -5.0, 5.0), mean=0.37, std=1.9)
    want, wc = _op(y_hat, y, 2, 0, bc, (9, -5.0, 5.0), mean=0.37, std=1.9)
    assert _same(flow, want) and torch.equal(counts, wc)
    assert metrics.flow_stats(y_hat, y)[1] is None
    assert _same(metrics.vorticity(y, u=2, v=0, dx=DX, dy=DY, boundary=("wall", "periodic")), _op_vorticity(y, 2, 0, bc))
    with pytest.raises(_lib.LnsError, match="shape"):
        metrics.flow_stats(y, y[:, :, :2])
    with pytest.raises(_lib.LnsError, match="two different channels"):
        metrics.flow_stats(y, y, u=1, v=1)
    with pytest.raises(_lib.LnsError, match="two different channels"):
        metrics.vorticity(y, u=0, v=3)
    with pytest.raises(_lib.LnsError, match="finite and positive"):
        metrics.flow_stats(y, y, dx=0.0)


# ---- the streaming calls ------------------------------------------------------------------------------------------------
VHIST = (32, -8.0, 8.0)
FLOW_KW = dict(u=0, v=1, dx=DX, dy=DY, boundary="auto")


def _reference(eng, out, yd, steps, vhist, norm):
    idx = list(range(T)) if steps is None else list(steps)
    flow, counts = eng.flow_stats(out[:, idx].contiguous(), yd[:, idx].contiguous(), vort_hist=vhist, **FLOW_KW, **norm)
    torch.cuda.synchronize()
    return idx, flow, counts


@pytest.mark.parametrize("case", ["ns2d_mini", "sw_half_periodic", "twophase_cond"])
def test_streaming_flow_same_bits_as_the_op_on_the_stored_rollout(case):
    teg._need_gpu()
    from lns_amd import metrics
    args, model, eng, xd, yd, pd, norm, denorm, y = teg._setup(case)
    out, f_ref, s_ref = teg._two_call(eng, xd, yd, pd, norm)
    bc = metrics.flow_boundary("auto", eng.cfg)
    assert bc == {"ns2d_mini": (0, 0), "sw_half_periodic": (1, 0), "twophase_cond": (1, 1)}[case]
    vort_ref = eng.vorticity(out[:, list(KEEP)].contiguous(), **FLOW_KW, **norm)
    shist = tes._hist_of(args)
    for steps, keep, vhist, stats_steps, spectrum_steps in (((0, 3, 4), KEEP, VHIST, (1, 2), (1, 3)), (None, (), None, (), ()),
                                                            ((2,), KEEP, None, None, ()), (None, (), VHIST, (), (0,))):
        idx, ref, cref = _reference(eng, out, yd, steps, vhist, norm)
        r = eng.rollout_eval_flow(xd, yd, param=pd, keep_steps=keep, flow_steps=steps, vort_hist=vhist, stats_steps=stats_steps,
                                  hist=shist if stats_steps != () else None, spectrum_steps=spectrum_steps, **FLOW_KW, **norm)
        torch.cuda.synchronize()
        what = (case, steps, keep, vhist, stats_steps, spectrum_steps)
        assert r.flow.shape == (B, len(idx), 12) and list(r.steps) == idx
        assert _same(r.flow, ref), what
        if vhist is None:
            assert r.hist is None
        else:
            assert torch.equal(r.hist, cref) and int(cref.sum()) == 2 * B * len(idx) * args.Ly * args.Lx, what
        assert _same(r.frame, f_ref) and _same(r.seq, s_ref), what
        if keep:
            assert _same(r.frames, out[:, list(keep)].contiguous()) and _same(r.vort_frames, vort_ref), what
        else:
            assert r.frames is None and r.vort_frames is None
        if stats_steps == ():
            assert r.stats is None and r.stats_hist is None and list(r.stats_steps) == []
        else:
            st = eng.rollout_eval_stats(xd, yd, param=pd, stats_steps=stats_steps, hist=shist, **norm)
            torch.cuda.synchronize()
            assert list(r.stats_steps) == list(st.stats_steps) and _same(r.stats, st.stats) and torch.equal(r.stats_hist, st.hist), what
        if spectrum_steps == ():
            assert r.spectra is None and list(r.spectrum_steps) == []
        else:
            sp = eng.rollout_eval_spectrum(xd, yd, param=pd, spectrum_steps=spectrum_steps, **norm)
            torch.cuda.synchronize()
            assert list(r.spectrum_steps) == list(sp.spectrum_steps) and _same(r.spectra, sp.spectra), what
        eng.check_finite(B, xd.device)
    # kept frames without their vorticity
    r = eng.rollout_eval_flow(xd, yd, param=pd, keep_steps=KEEP, vort_frames=False, **FLOW_KW, **norm)
    torch.cuda.synchronize()
    assert r.vort_frames is None and _same(r.frames, out[:, list(KEEP)].contiguous())
    # the diagnostics are what the statement says of the same stored fields
    _, ref, cref = _reference(eng, out, yd, None, VHIST, norm)
    kw = dict(u=0, v=1, dx=DX, dy=DY, bc=bc, **norm)
    assert _same(ref, fl.statement32(out, yd, **kw))
    assert np.array_equal(cref.cpu().numpy().astype(np.int64), fl.counts(out, yd, *VHIST, **kw))
    assert _same(vort_ref, fl.vorticity32(out[:, list(KEEP)].contiguous(), **kw))


def test_streaming_flow_does_not_depend_on_scheduling_options():
    teg._need_gpu()
    args, model, eng, xd, yd, pd, norm, denorm, y = teg._setup("ns2d_mini")
    out, f_ref, s_ref = teg._two_call(eng, xd, yd, pd, norm)
    shist = tes._hist_of(args)
    steps, stats_steps, spectrum_steps = (0, 4), (1, 4), (3,)          # groups of 1, 2, 3 steps: some select nothing
    _, ref, cref = _reference(eng, out, yd, steps, VHIST, norm)
    st_ref, sc_ref = eng.field_stats(out[:, list(stats_steps)].contiguous(), yd[:, list(stats_steps)].contiguous(), hist=shist, **norm)
    sp_ref = eng.energy_spectrum(out[:, list(spectrum_steps)].contiguous(), yd[:, list(spectrum_steps)].contiguous(), **norm)
    keep_ref = out[:, list(KEEP)].contiguous()
    vort_ref = eng.vorticity(keep_ref, **FLOW_KW, **norm)

    def check(tag):
        r = eng.rollout_eval_flow(xd, yd, param=pd, keep_steps=KEEP, flow_steps=steps, vort_hist=VHIST, stats_steps=stats_steps,
                                  hist=shist, spectrum_steps=spectrum_steps, **FLOW_KW, **norm)
        torch.cuda.synchronize()
        assert _same(r.flow, ref) and torch.equal(r.hist, cref) and _same(r.vort_frames, vort_ref), tag
        assert _same(r.stats, st_ref) and torch.equal(r.stats_hist, sc_ref) and _same(r.spectra, sp_ref), tag
        assert _same(r.frame, f_ref) and _same(r.seq, s_ref) and _same(r.frames, keep_ref), tag
    for dg in (1, 2, 3, 0):
        for ds in (1, 2, 3, 4):
            for ov in (0, 1):
                eng.set_option("decode_group", dg)
                eng.set_option("decode_streams", ds)
                eng.set_option("overlap", ov)
                check((dg, ds, ov))
    eng.set_option("decode_group", 2)
    eng.timing_enable(True)                                        # diagnostics mode: everything on the caller's stream
    check("timing")
    eng.timing_enable(False)


@pytest.mark.parametrize("case", ["ns2d_mini", "sw_half_periodic", "twophase_cond"])
def test_chunked_latent_calls_reproduce_the_one_call_result(case):
    teg._need_gpu()
    args, model, eng, xd, yd, pd, norm, denorm, y = teg._setup(case)
    shist = tes._hist_of(args)
    one = eng.rollout_eval_flow(xd, yd, param=pd, keep_steps=KEEP, vort_hist=VHIST, stats_steps=None, hist=shist, spectrum_steps=None,
                                **FLOW_KW, **norm)
    torch.cuda.synchronize()
    z0 = eng.encode(xd) if not eng.cfg.cond_encoder else eng.encode(xd, pd)
    a = eng.rollout_latent_eval_flow(z0, yd, steps=3, t0=0, param=pd, keep_steps=(0,), flow_steps=(0, 1, 2), vort_hist=VHIST,
                                     stats_steps=None, hist=shist, spectrum_steps=None, **FLOW_KW, **norm)
    b = eng.rollout_latent_eval_flow(a.z_last, yd, steps=2, t0=3, param=pd, keep_steps=(0, 1), flow_steps=None, vort_hist=VHIST,
                                     stats_steps=None, hist=shist, spectrum_steps=None, frame=a.frame, seq=a.seq, **FLOW_KW, **norm)
    torch.cuda.synchronize()
    assert _same(torch.cat([a.flow, b.flow], 1), one.flow) and torch.equal(torch.cat([a.hist, b.hist], 1), one.hist), case
    assert _same(torch.cat([a.vort_frames, b.vort_frames], 1), one.vort_frames) and _same(torch.cat([a.frames, b.frames], 1), one.frames)
    assert _same(torch.cat([a.stats, b.stats], 1), one.stats) and torch.equal(torch.cat([a.stats_hist, b.stats_hist], 1), one.stats_hist)
    assert _same(torch.cat([a.spectra, b.spectra], 1), one.spectra)
    assert _same(b.frame, one.frame) and _same(b.seq, one.seq)
    assert list(a.steps) == [0, 1, 2] and list(b.steps) == [0, 1]
    # a selection inside the chunk is relative to the chunk
    c = eng.rollout_latent_eval_flow(a.z_last, yd, steps=2, t0=3, param=pd, flow_steps=(1,), frame=a.frame, seq=a.seq, **FLOW_KW, **norm)
    torch.cuda.synchronize()
    assert _same(c.flow, one.flow[:, 4:5].contiguous()) and c.hist is None and c.vort_frames is None and c.stats is None and c.spectra is None


def test_workspace_is_the_evaluation_workspace():
    teg._need_gpu()
    from lns_amd import _lib, engine
    args, model, eng, xd, yd, pd, norm, denorm, y = teg._setup("ns2d_mini")
    L, h = eng._L, eng._h
    n1 = ctypes.c_size_t(0)
    assert L.lns_rollout_eval_workspace_bytes(h, B, ctypes.byref(n1)) == 0
    C = args.in_channels
    spec = engine.eval_spec(C, **norm)
    fs = engine.flow_spec(0, 1, DX, DY, "auto", VHIST, cfg=eng.cfg)
    frame = torch.empty((B, T, C), dtype=torch.float32, device="cuda")
    seq = torch.empty((B, C), dtype=torch.float32, device="cuda")
    flow = torch.empty((B, T, 12), dtype=torch.float32, device="cuda")
    counts = torch.empty((B, T, 2, VHIST[0] + 2), dtype=torch.int32, device="cuda")
    ws = torch.empty(n1.value, dtype=torch.uint8, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    f = _lib.LnsEvalFlow()
    f.size = ctypes.sizeof(_lib.LnsEvalFlow)
    f.n_flow, f.flow_steps_host, f.fspec = T, (ctypes.c_int * T)(*range(T)), ctypes.pointer(fs)
    f.flow_out, f.hist_out = flow.data_ptr(), counts.data_ptr()

    def run(nbytes):
        return L.lns_rollout_eval_flow(h, xd.data_ptr(), None, yd.data_ptr(), B, T, ctypes.byref(spec), frame.data_ptr(),
                                       seq.data_ptr(), None, 0, None, ws.data_ptr(), nbytes, stream, None, ctypes.byref(f))
    assert run(n1.value - 1) == _lib.LNS_ENOMEM and "workspace" in L.lns_last_error(h).decode()
    assert run(n1.value) == 0
    torch.cuda.synchronize()
    out, f_ref, s_ref = teg._two_call(eng, xd, yd, pd, norm)
    _, ref, cref = _reference(eng, out, yd, None, VHIST, norm)
    assert _same(flow, ref) and torch.equal(counts, cref) and _same(frame, f_ref) and _same(seq, s_ref)


@pytest.mark.parametrize("case", ["ns2d_mini", "twophase_cond"])
def test_validate_flow_is_the_hand_written_composition(case):
    teg._need_gpu()
    from lns_amd import engine, metrics
    args, model, eng, xd, yd, pd, norm, denorm, y = teg._setup(case)
    out, f_ref, s_ref = teg._two_call(eng, xd, yd, pd, norm)
    extra = (pd,) if pd is not None else ()
    names = tuple(metrics.FLOW_BOUNDARIES[b] for b in metrics.flow_boundary("auto", eng.cfg))
    v = model.validate_flow(xd, yd, *extra, flow_steps=slice(None, None, 2), dx=DX, dy=DY, vort_hist=VHIST, spectrum_steps=(1, 4),
                            keep_steps=KEEP, **norm)
    torch.cuda.synchronize()
    assert isinstance(v, engine.EvalFlow) and list(v.steps) == [0, 2, 4] and list(v.spectrum_steps) == [1, 4] and v.stats is None
    flow, counts = metrics.flow_stats(out[:, [0, 2, 4]].contiguous(), yd[:, [0, 2, 4]].contiguous(), dx=DX, dy=DY, boundary=names,
                                      vort_hist=VHIST, **norm)
    assert _same(v.flow, flow) and torch.equal(v.hist, counts)
    assert _same(v.vort_frames, metrics.vorticity(out[:, list(KEEP)].contiguous(), dx=DX, dy=DY, boundary=names, **norm))
    assert _same(v.spectra, metrics.energy_spectrum(out[:, [1, 4]].contiguous(), yd[:, [1, 4]].contiguous(), **norm))
    assert _same(v.frame, f_ref) and _same(v.seq, s_ref) and _same(v.frames, out[:, list(KEEP)].contiguous())
    # the defaults: every step, unit spacings, no histogram, no statistics, no spectra, no kept frames
    d = model.validate_flow(xd, yd, *extra, **norm)
    torch.cuda.synchronize()
    assert list(d.steps) == list(range(T)) and d.hist is None and d.spectra is None and d.frames is None and d.vort_frames is None
    assert _same(d.flow, metrics.flow_stats(out, yd, boundary=names, **norm)[0])
    with pytest.raises(TypeError):
        model.validate_flow(xd, yd, *extra, 1.0, **norm)

"""GPU (-m gpu): the streaming validation rollout (lns_rollout_eval / lns_rollout_latent_eval, include/lns.h) against
the two-call path it replaces -- `Engine.rollout` then `metrics.relative_l2` -- BIT FOR BIT, against the CPU oracle, and
the `*_stable` fixtures in the reference's own per-(b, t, c) metric.

Why equality and not a tolerance: the decoder writes the same values wherever its output pointer aims, and the
group-scoring kernel runs the per-plane reduction of the metric kernels (one shared device function, same thread
striding, same wave and block sums) into the same [B][T][C][2] partials that the unchanged finish kernel reads."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from helpers import load_golden, case_args, case_variant  # noqa: E402

pytestmark = pytest.mark.gpu

B, T = 3, 5
KEEP = (0, 3, 4)
FAMILY_CASES = ["ns2d_mini", "sw_half_periodic", "sw_96x192x5", "twophase", "twophase_cond"]
TWOPHASE_STATS = (0.013, 0.21, 310.0, 180.0)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _norm(args):
    """The family's own denormalisation: (keyword arguments of relative_l2 / rollout_eval, oracle denorm or None)."""
    import lns_oracle
    from lns_amd import metrics
    C = args.in_channels
    if args.family == "ns2d":
        return dict(mean=0.37, std=1.9), None
    if args.family.startswith("sw"):
        mean = [0.4, -0.2, 9.5, 0.15, -1.1][:C]
        std = [2.1, 1.7, 0.6, 1.3, 0.9][:C]
        return dict(mean=mean, std=std), (lambda a: lns_oracle.denormalize_channels(a, mean, std))
    return metrics.twophase_spec(*TWOPHASE_STATS), (lambda a: lns_oracle.denormalize_twophase(a, *TWOPHASE_STATS))


def _setup(case, variant=None):
    import gpu_checks as gc
    from lns_amd import filler
    meta, _ = load_golden(case)
    args = case_args(meta)
    model, _ = gc.build_models(args, meta["weight_seed"], variant)
    seed = meta["input_seed"]
    x = filler.normal("x", (B, args.in_channels, args.Ly, args.Lx), seed)
    param = filler.uniform01("param", B, seed).astype(np.float32) if args.family == "twophase_cond" else None
    norm, denorm = _norm(args)
    y = filler.normal("y", (B, T, args.in_channels, args.Ly, args.Lx), seed).astype(np.float32)
    m0 = norm["mean"] if isinstance(norm["mean"], float) else norm["mean"][0]
    s0 = norm["std"] if isinstance(norm["std"], float) else norm["std"][0]
    y[0, 0, 0] = -m0 / s0                                        # denormalises to ~0: the eps clamp
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    pd = torch.from_numpy(param).cuda() if param is not None else None
    return args, model, model._engine(xd), xd, yd, pd, norm, denorm, y


def _two_call(eng, xd, yd, pd, norm):
    from lns_amd import metrics
    out = eng.rollout(xd, T, param=pd)
    f, s = metrics.relative_l2(out, yd, **norm)
    torch.cuda.synchronize()
    return out, f, s


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("case", FAMILY_CASES)
def test_rollout_eval_same_bits_as_the_two_call_path(case):
    """frame / seq bitwise equal to relative_l2(rollout(x, T), y), kept frames bitwise equal to rollout(...)[:, keep];
    and (tolerances of test_metric_rel_l2_matches_oracle) equal to the oracle's rollout_metrics on that rollout."""
    _need_gpu()
    import lns_oracle
    args, model, eng, xd, yd, pd, norm, denorm, y = _setup(case)
    out, f_ref, s_ref = _two_call(eng, xd, yd, pd, norm)
    for _ in range(2):
        f, s, frames = eng.rollout_eval(xd, yd, param=pd, keep_steps=KEEP, **norm)
        torch.cuda.synchronize()
        assert f.shape == (B, T, args.in_channels) and s.shape == (B, args.in_channels)
        assert _same(f, f_ref) and _same(s, s_ref), case
        assert _same(frames, out[:, list(KEEP)].contiguous()), case
    eng.check_finite(B, xd.device)
    # without kept frames, and a single output
    f2, s2, none = eng.rollout_eval(xd, yd, param=pd, **norm)
    assert none is None and _same(f2, f_ref) and _same(s2, s_ref)
    # the oracle on the same decoded rollout
    kw = dict(denorm=denorm) if denorm is not None else dict(mean=norm["mean"], std=norm["std"])
    fo, so = lns_oracle.rollout_metrics(out.cpu().numpy(), y, **kw)
    f64, s64 = f.cpu().numpy().astype(np.float64), s.cpu().numpy().astype(np.float64)
    big = fo > 1e3                                               # clamp-dominated entries: compare in log scale
    assert np.allclose(f64[~big], fo[~big], rtol=2e-5, atol=1e-7)
    assert np.allclose(np.log(f64[big]), np.log(fo[big]), rtol=1e-2) if big.any() else True
    assert np.allclose(s64, so, rtol=2e-5, atol=1e-7)


def test_rollout_eval_does_not_depend_on_scheduling_options():
    _need_gpu()
    args, model, eng, xd, yd, pd, norm, denorm, y = _setup("ns2d_mini")
    out, f_ref, s_ref = _two_call(eng, xd, yd, pd, norm)
    keep_ref = out[:, list(KEEP)].contiguous()
    for dg in (1, 2, 0):
        for ds in (1, 3):
            for ov in (0, 1):
                eng.set_option("decode_group", dg)
                eng.set_option("decode_streams", ds)
                eng.set_option("overlap", ov)
                for _ in range(2):
                    f, s, frames = eng.rollout_eval(xd, yd, param=pd, keep_steps=KEEP, **norm)
                    torch.cuda.synchronize()
                    assert _same(f, f_ref) and _same(s, s_ref) and _same(frames, keep_ref), (dg, ds, ov)
    eng.set_option("decode_group", 2)
    eng.timing_enable(True)                                      # diagnostics mode: everything on the caller's stream
    f, s, frames = eng.rollout_eval(xd, yd, param=pd, keep_steps=KEEP, **norm)
    torch.cuda.synchronize()
    eng.timing_enable(False)
    assert _same(f, f_ref) and _same(s, s_ref) and _same(frames, keep_ref)


def test_rollout_eval_scalar_form_on_odd_planes():
    """61 x 121 planes: every other plane of a [B,T,C,H,W] tensor is not 16-byte aligned, where the metric kernel sums in
    element order instead of the float4 order; the group kernel follows the truth plane's alignment like it does."""
    _need_gpu()
    args, model, eng, xd, yd, pd, _, _, _ = _setup("twophase")
    norm = dict(mean=0.37, std=1.9)
    out, f_ref, s_ref = _two_call(eng, xd, yd, pd, norm)
    for dg in (1, 2):
        eng.set_option("decode_group", dg)
        f, s, _ = eng.rollout_eval(xd, yd, param=pd, **norm)
        torch.cuda.synchronize()
        assert _same(f, f_ref) and _same(s, s_ref), dg


@pytest.mark.parametrize("case", ["ns2d_mini", "twophase_cond"])
def test_rollout_latent_eval_in_chunks_equals_one_call(case):
    _need_gpu()
    args, model, eng, xd, yd, pd, norm, denorm, y = _setup(case)
    out, f_ref, s_ref = _two_call(eng, xd, yd, pd, norm)
    z0 = eng.encode(xd) if not eng.cfg.cond_encoder else eng.encode(xd, pd)
    f1, s1, fr1, _ = eng.rollout_latent_eval(z0, yd, param=pd, keep_steps=KEEP, **norm)
    torch.cuda.synchronize()
    assert _same(f1, f_ref) and _same(s1, s_ref) and _same(fr1, out[:, list(KEEP)].contiguous())
    f, s, fra, z2 = eng.rollout_latent_eval(z0, yd, steps=2, t0=0, param=pd, keep_steps=(0,), **norm)
    f, s, frb, z5 = eng.rollout_latent_eval(z2, yd, steps=3, t0=2, param=pd, keep_steps=(1, 2), frame=f, seq=s, **norm)
    torch.cuda.synchronize()
    assert _same(f, f_ref) and _same(s, s_ref), case
    assert _same(torch.cat([fra, frb], 1), out[:, list(KEEP)].contiguous())
    _, z_ref = eng.rollout_latent(z0, T, param=pd, to_x=False)
    assert _same(z5, z_ref)


def test_eval_workspace_is_appended_to_the_rollout_workspace():
    _need_gpu()
    from lns_amd import _lib, engine
    args, model, eng, xd, yd, pd, norm, denorm, y = _setup("ns2d_mini")
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
    # include/lns.h: the lns_prepare layout, then `decode_streams` frame buffers of decode_group * B * C * Ly * Lx floats
    # and the [B][eval_max_steps][C][2] partial sums, each rounded up to 256 bytes
    assert n1.value - up(n0.value) == ndec * up(kdec * B * C * HW * 4) + up(B * max_steps * C * 2 * 4)
    spec = engine.eval_spec(C, **norm)
    frame = torch.empty((B, T, C), dtype=torch.float32, device="cuda")
    seq = torch.empty((B, C), dtype=torch.float32, device="cuda")
    ws = torch.empty(n1.value, dtype=torch.uint8, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run(nbytes):
        return L.lns_rollout_eval(h, xd.data_ptr(), None, yd.data_ptr(), B, T, ctypes.byref(spec), frame.data_ptr(),
                                  seq.data_ptr(), None, 0, None, ws.data_ptr(), nbytes, stream)
    assert run(n1.value - 1) == _lib.LNS_ENOMEM and "workspace" in L.lns_last_error(h).decode()
    assert run(n1.value) == 0
    torch.cuda.synchronize()
    _, f_ref, s_ref = _two_call(eng, xd, yd, pd, norm)
    assert _same(frame, f_ref) and _same(seq, s_ref)
    # the rollout's own workspace is what it was, and lns_rollout runs in exactly that many bytes
    n2 = ctypes.c_size_t(0)
    assert L.lns_prepare(h, B, ctypes.byref(n2)) == 0 and n2.value == n0.value
    out = torch.empty((B, T, C, args.Ly, args.Lx), dtype=torch.float32, device="cuda")
    small = torch.empty(n0.value, dtype=torch.uint8, device="cuda")
    assert L.lns_rollout(h, xd.data_ptr(), None, B, T, 1, out.data_ptr(), None, small.data_ptr(), n0.value, stream) == 0
    assert L.lns_rollout(h, xd.data_ptr(), None, B, T, 1, out.data_ptr(), None, small.data_ptr(), n0.value - 1, stream) == _lib.LNS_ENOMEM
    torch.cuda.synchronize()
    assert _same(out, eng.rollout(xd, T))


@pytest.mark.parametrize("case", ["ns2d_mini", "twophase_cond"])
def test_validate_returns_the_rollout_eval_result(case):
    _need_gpu()
    from lns_amd._lib import LnsError
    args, model, eng, xd, yd, pd, norm, denorm, y = _setup(case)
    out, f_ref, s_ref = _two_call(eng, xd, yd, pd, norm)
    extra = (pd,) if pd is not None else ()
    f, s, frames = model.validate(xd, yd, *extra, keep_steps=KEEP, **norm)
    torch.cuda.synchronize()
    assert _same(f, f_ref) and _same(s, s_ref) and _same(frames, out[:, list(KEEP)].contiguous())
    f, s, frames = model.validate(xd.unsqueeze(1), yd, *extra, **norm)          # loaders that hand [B,1,C,H,W]
    assert frames is None and _same(f, f_ref) and _same(s, s_ref)
    with pytest.raises(LnsError, match="no CPU fallback"):
        model.validate(xd.cpu(), yd.cpu(), *extra, **norm)
    if pd is not None:
        with pytest.raises(TypeError):
            model.validate(xd, yd, **norm)


# The full-horizon fixtures in the reference's OWN metric: relative_lp_loss(reduce_dim=(3, 4)) per (b, stored step, c)
# of the engine's decoded (sub-sampled) field against the reference's fp32 and fp64 runs.  The pooled rel-L2 of
# test_full_horizon_rollout_vs_reference_stable can hide one bad channel of one trajectory; a cell cannot.
# Gate: the project's 1e-4.  The reference's own fp32-vs-fp64 worst cell on these fixtures is 1.8e-5 (NS2d T256),
# 4.3e-6 (SW T64) and 1.4e-5 (two-phase conditional T128), computed from the fixtures alone, so the gate leaves room.
CELL_TOL = 1e-4


def _cells(f, g):
    f, g = np.asarray(f, np.float64), np.asarray(g, np.float64)
    return np.sqrt(((f - g) ** 2).sum((-1, -2)) / np.maximum((g ** 2).sum((-1, -2)), 1e-8))


@pytest.mark.parametrize("case", ["sw_96x192x5_T64_stable", "twophase_cond_T128_stable", "ns2d_128_T256_stable"])
def test_stable_fixtures_per_cell_relative_l2(case):
    _need_gpu()
    import gpu_checks as gc
    from helpers import case_inputs
    meta, g = load_golden(case)
    args = case_args(meta)
    model, _ = gc.build_models(args, meta["weight_seed"], case_variant(meta))
    x, param = case_inputs(meta, args)
    xd = torch.from_numpy(x).cuda()
    extra = (torch.from_numpy(param).cuda(),) if param is not None else ()
    dec = model.predict(xd, meta["T"], *extra, to_x=True)
    torch.cuda.synchronize()
    dec = dec.cpu().numpy()
    sub = meta["sub"]
    mine = np.stack([dec[:, s - 1][..., ::sub, ::sub] for s in meta["steps"]], 1)      # [B, stored steps, C, h, w]
    e32, e64 = _cells(mine, g["dec"]), _cells(mine, g["dec_f64"])
    ref = _cells(g["dec"], g["dec_f64"])
    for name, e in (("vs fp32 run", e32), ("vs fp64 run", e64), ("reference fp32 vs fp64", ref)):
        b, i, c = np.unravel_index(int(e.argmax()), e.shape)
        print("%s %s: worst cell %.3e at (b=%d, step=%d, c=%d)" % (case, name, e.max(), b, meta["steps"][i], c))
    assert ref.max() < CELL_TOL                                   # the premise: the reference itself sits inside the gate
    assert e32.max() < CELL_TOL and e64.max() < CELL_TOL, (float(e32.max()), float(e64.max()))

"""GPU (-m gpu): the ensemble rollout (lns_rollout_latent_ensemble, lns_op_ensemble_stats, include/lns.h;
Engine.rollout_latent_ensemble / ensemble_stats, LatentDynamics.predict_ensemble).

The reference of every case is the fp32 statement of include/lns.h, written below in torch as explicit elementwise ops
in a loop over the members (no `sum`, no `var`; every op is its own kernel, so nothing is fused), applied to the frames
the existing `rollout_latent` at batch B * M produces.  The mean is held to it BIT FOR BIT: an element's result depends on
its M inputs only and the order is fixed, so there is nothing to tolerate.  The variance is held to the same bits and,
against float64 of the same fp32 frames, to the project's rule max(2e-7, 3 x own): `own` is the float64 distance of
torch.var(frames, dim=1, unbiased=True) computed in fp32 on the device in the same test, 2e-7 the floor the float32
fixtures are held to in tests/test_train_reference_cpu.py; both in max |diff| / max |ref| and in rel-L2."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from helpers import load_golden, case_args  # noqa: E402

pytestmark = pytest.mark.gpu

B, M, T = 2, 3, 7
NOISE = 0.05
KEEP_SETS = ([0], [6], [1, 4, 6], [0, 1, 2, 3, 4, 5, 6], [2, 3], [0, 2, 3, 4, 6])   # tests/test_rollout_select_gpu.py's, plus 3 + 2
DEFAULTS = dict(decode_group=1, decode_streams=3, overlap=1)
FLOOR = 2e-7

_cases = {}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def statement(frames):
    """frames [B, M, ...] fp32 on the device -> (mean, var or None): the statement of include/lns.h, one rounded fp32 op
    after the other.  The divisors are device tensors: torch turns a division by a host scalar into a multiplication by
    its reciprocal, which is not the correctly rounded quotient."""
    m_count = frames.shape[1]
    fm = torch.full_like(frames[:, 0], float(m_count))
    s = frames[:, 0].clone()
    for m in range(1, m_count):
        s = s + frames[:, m]
    mean = s / fm
    if m_count < 2:
        return mean, None
    sd = torch.zeros_like(mean)
    q = torch.zeros_like(mean)
    for m in range(m_count):
        d = frames[:, m] - mean
        p = d * d
        sd = sd + d
        q = q + p
    c = sd * sd
    k = c / fm
    n = q - k
    return mean, n / torch.full_like(mean, float(m_count - 1))


def var_rule(var, frames, what):
    """max(2e-7, 3 x own) against float64 of the same frames, in both measures -> the two ratios ours / bound."""
    ref = frames.double().var(dim=1, unbiased=True)
    own = torch.var(frames, dim=1, unbiased=True)

    def errs(a):
        d = a.double() - ref
        return float(d.abs().max() / ref.abs().max()), float(d.norm() / ref.norm())
    ours, owns = errs(var), errs(own)
    ratios = [o / max(FLOOR, 3.0 * w) for o, w in zip(ours, owns)]
    print("%s: rel-max %.3e (own %.3e) rel-L2 %.3e (own %.3e) -> %.3f %.3f of the bound" % (what, ours[0], owns[0], ours[1], owns[1], *ratios))
    assert ours[0] <= max(FLOOR, 3.0 * owns[0]) and ours[1] <= max(FLOOR, 3.0 * owns[1]), (what, ours, owns)
    return ratios


# ---- the op ------------------------------------------------------------------------------------------------------------
SENTINEL = -12345.0


def _op(frames_flat, b, m, per, off_f=0, off_m=0, off_v=0, want_var=True):
    """lns_op_ensemble_stats through ctypes with each buffer optionally one float off a 16-byte boundary; the outputs sit
    between sentinels that must survive."""
    from lns_amd import _lib
    L = _lib.lib()
    n_in, n_out = b * m * per, b * per
    fbuf = torch.empty(n_in + 4, device="cuda")
    assert fbuf.data_ptr() % 16 == 0
    f = fbuf[off_f:off_f + n_in]
    f.copy_(frames_flat)
    outs = []
    for off in (off_m, off_v):
        buf = torch.full((n_out + 8,), SENTINEL, device="cuda")
        assert buf.data_ptr() % 16 == 0
        outs.append((buf, buf[4 + off:4 + off + n_out]))
    (mbuf, mean), (vbuf, var) = outs
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.lns_op_ensemble_stats(f.data_ptr(), b, m, per, mean.data_ptr(), var.data_ptr() if want_var else None, stream)
    assert rc == 0, L.lns_create_error()
    for buf, view, off in ((mbuf, mean, off_m), (vbuf, var, off_v)):
        assert bool((buf[:4 + off] == SENTINEL).all()) and bool((buf[4 + off + n_out:] == SENTINEL).all())
    if not want_var:
        assert bool((vbuf == SENTINEL).all())
    return mean.view(b, per), (var.view(b, per) if want_var else None)


def test_op_mean_and_variance_have_the_bits_of_the_statement():
    """B in {1, 3} x M in {1, 2, 3, 7, 33} x per in {1, 3, 4, 5, 1027} (below, at and above the float4 width; 1027 = two
    blocks and a tail), all pointers aligned (per 4: the float4 path) and frames / mean / var each one float off a
    16-byte boundary (the element-wise path): equal bits, nothing written outside the outputs.  M = 1 returns the input."""
    _need_gpu()
    from lns_amd import _lib
    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    for b in (1, 3):
        for m in (1, 2, 3, 7, 33):
            for per in (1, 3, 4, 5, 1027):
                frames = torch.randn((b, m, per), device="cuda", generator=g) * 3.0 + 0.5
                ref_mean, ref_var = statement(frames)
                for offs in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
                    mean, var = _op(frames.reshape(-1), b, m, per, *offs, want_var=m > 1)
                    assert _same(mean, ref_mean), (b, m, per, offs)
                    if m > 1:
                        assert _same(var, ref_var), (b, m, per, offs)
                    else:
                        assert _same(mean, frames[:, 0])
    # 4096 elements per row, aligned: every thread of four blocks on the float4 path; and var refused for M = 1
    frames = torch.randn((2, 5, 4096), device="cuda", generator=g)
    mean, var = _op(frames.reshape(-1), 2, 5, 4096)
    ref_mean, ref_var = statement(frames)
    assert _same(mean, ref_mean) and _same(var, ref_var)
    one = torch.zeros(8, device="cuda")
    assert _lib.lib().lns_op_ensemble_stats(one.data_ptr(), 2, 1, 4, one.data_ptr(), one.data_ptr(), None) == _lib.LNS_EINVAL


def test_op_variance_against_float64():
    """Measured on MI355X, ours / max(2e-7, 3 x own) as (rel-max, rel-L2), worst over M in {2, 7, 33}: normal 0.572, 0.449;
    mean 1e3 / spread 1e-2 below 0.001 in both (ours 6.6e-08 against torch.var's own 5.1e-03); 1e-12 0.439, 0.436; 1e12 0.579,
    0.447.  At M = 2 the kernel's error equals torch's own (0.333 of the bound).  Each case prints its figures.
    All members equal: the values are rounded to bfloat16 (8 significant bits), so every partial sum k * v, k <= 33, is
    exact in fp32 (8 + 6 bits), the mean is exactly v, every d_m is exactly 0 and so is the variance."""
    _need_gpu()
    from lns_amd import config, engine
    eng = engine.Engine(engine.make_config(config.preset("ns2d_mini"), ae_prefix="vq_ae.", prop_prefix="propagator."))
    g = torch.Generator(device="cuda")
    g.manual_seed(12)
    b, per = 3, 1027
    for m in (2, 7, 33):
        base = torch.randn((b, m, per), device="cuda", generator=g)
        for what, frames in (("normal", base), ("mean 1e3 spread 1e-2", 1e3 + 1e-2 * base), ("1e-12", 1e-12 * base),
                             ("1e12", 1e12 * base)):
            frames = frames.contiguous()
            mean, var = eng.ensemble_stats(frames)
            ref_mean, ref_var = statement(frames)
            assert _same(mean, ref_mean) and _same(var, ref_var), (what, m)
            assert bool((var >= 0).all())
            var_rule(var, frames, "M=%d %s" % (m, what))
        v = base[:, :1].to(torch.bfloat16).to(torch.float32)
        mean, var = eng.ensemble_stats(v.expand(b, m, per).contiguous())
        assert _same(mean, v[:, 0]) and bool((var == 0).all()), m
    # one NaN and one inf, each in a single member of a single (b, pixel): that element alone is not finite
    frames = torch.randn((b, 7, per), device="cuda", generator=g)
    frames[1, 3, 500] = float("nan")
    frames[2, 6, 1026] = float("inf")
    mean, var = eng.ensemble_stats(frames)
    bad = torch.zeros((b, per), dtype=torch.bool, device="cuda")
    bad[1, 500] = True
    bad[2, 1026] = True
    assert torch.equal(~torch.isfinite(mean), bad) and torch.equal(~torch.isfinite(var), bad)
    assert bool(torch.isnan(mean[1, 500])) and float(mean[2, 1026]) == float("inf")


# ---- the engine --------------------------------------------------------------------------------------------------------
def _options(eng, **kw):
    for k, v in dict(DEFAULTS, **kw).items():
        if eng.options.get(k, DEFAULTS[k]) != v:
            eng.set_option(k, v)


def _case(name):
    """(args, model, engine, x, z [B, M, c, h, w], param [B, M] or None, {T: reference}) -- built once per preset.  The
    reference of T steps is the statement over the members of rollout_latent at batch B * M, for all T steps: the statement
    is elementwise, so a keep set's reference is its slice.  Never written afterwards."""
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
        # a parameter ensemble: every member its own value
        pd = torch.from_numpy(filler.uniform01("param", B * M, seed).astype(np.float32)).cuda().view(B, M) \
            if args.family == "twophase_cond" else None
        _cases[name] = (args, model, eng, xd, z, pd, {})
    return _cases[name]


def _ref(name, steps):
    args, model, eng, xd, z, pd, refs = _case(name)
    if steps not in refs:
        _options(eng)
        full, z_last = eng.rollout_latent(z.view((B * M,) + tuple(z.shape[2:])), steps, param=None if pd is None else pd.reshape(-1))
        torch.cuda.synchronize()
        frames = full.view((B, M) + tuple(full.shape[1:]))
        mean, var = statement(frames)
        refs[steps] = (frames, mean, var, z_last.view_as(z))
    return refs[steps]


def _check(name, steps, keep, twice=False):
    args, model, eng, xd, z, pd, _ = _case(name)
    frames, mean_ref, var_ref, z_last_ref = _ref(name, steps)
    for _ in range(2 if twice else 1):
        mean, var, z_last = eng.rollout_latent_ensemble(z, steps, param=pd, keep_steps=keep, return_last=True)
        torch.cuda.synchronize()
        assert mean.shape == (B, len(keep), args.in_channels, args.Ly, args.Lx) == var.shape
        assert _same(mean, mean_ref[:, keep]), (name, keep, eng.options)
        assert _same(var, var_ref[:, keep]), (name, keep, eng.options)
        assert _same(z_last, z_last_ref), (name, keep, eng.options)
    return mean, var, z_last


GRID = [("ns2d_mini", dg, ds, ov) for dg in (1, 2, 3, 0) for ds in (1, 3) for ov in (0, 1)] + \
       [(c, dg, ds, 1) for c in ("twophase_cond", "sw_half_periodic") for dg in (1, 2) for ds in (1, 3)]


@pytest.mark.parametrize("case,dg,ds,ov", GRID)
def test_ensemble_has_the_bits_of_the_statement_over_the_member_rollouts(case, dg, ds, ov):
    """mean[:, i] == statement(rollout_latent(z.view(B * M, ...), T)[:, keep[i]]) bit for bit, for every scheduling option;
    var and z_last are those of the default options (and of the statement / the member rollout) in every cell.
    twophase_cond runs with one parameter value per member."""
    _need_gpu()
    eng = _case(case)[2]
    _ref(case, T)
    _options(eng)
    defaults = {tuple(keep): _check(case, T, keep) for keep in KEEP_SETS}
    try:
        _options(eng, decode_group=dg, decode_streams=ds, overlap=ov)
        for keep in KEEP_SETS:
            got = _check(case, T, keep)
            for a, b in zip(got, defaults[tuple(keep)]):
                assert _same(a, b), (case, keep, eng.options)
    finally:
        _options(eng)


@pytest.mark.parametrize("case", ["ns2d_mini", "twophase_cond", "sw_half_periodic"])
def test_ensemble_variance_against_float64(case):
    """The variance of the decoded member fields under the rule of the op test (M = 3, all 7 steps).  Measured on MI355X
    (rel-max, rel-L2 of the bound): ns2d_mini 0.331, 0.253; twophase_cond 0.353, 0.254; sw_half_periodic 0.195, 0.254."""
    _need_gpu()
    args, model, eng, xd, z, pd, _ = _case(case)
    frames = _ref(case, T)[0]
    _options(eng)
    mean, var = eng.rollout_latent_ensemble(z, T, param=pd)
    var_rule(var, frames, case)
    # the mean alone, and a preallocated output
    out = torch.full_like(mean, float("nan"))
    assert eng.rollout_latent_ensemble(z, T, param=pd, return_var=False, out=out) is out and _same(out, mean)


def test_one_member_is_the_selected_rollout():
    _need_gpu()
    from lns_amd import _lib
    from lns_amd._lib import LnsError
    args, model, eng, xd, z, pd, _ = _case("ns2d_mini")
    _options(eng)
    keep = [1, 4, 6]
    z1 = z[:, :1].contiguous()
    sel, z_last = eng.rollout_latent(z1[:, 0].contiguous(), T, keep_steps=keep)
    mean, last = eng.rollout_latent_ensemble(z1, T, keep_steps=keep, return_var=False, return_last=True)
    torch.cuda.synchronize()
    assert _same(mean, sel) and _same(last[:, 0], z_last)
    with pytest.raises(LnsError, match="at least 2 members"):
        eng.rollout_latent_ensemble(z1, T, keep_steps=keep)
    L, h = eng._L, eng._h
    ws = eng._ws[(B, z.device)]
    out = torch.full_like(mean, SENTINEL)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.lns_rollout_latent_ensemble(h, z1.data_ptr(), None, B, 1, T, (ctypes.c_int * 3)(*keep), 3, out.data_ptr(), out.data_ptr(),
                                       None, ws.data_ptr(), ws.numel(), stream)
    assert rc == _lib.LNS_EINVAL and L.lns_last_error(h).decode() == "var_out needs M >= 2"
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


def test_ring_groups_and_frame_buffers_are_reused():
    """The two keep sets of tests/test_rollout_select_gpu.py::test_ring_groups_are_reused_under_selection (more kept groups
    than ring groups, and than frame buffers: a frame buffer is reduced before the next decode on its stream overwrites
    it), twice in a row on one workspace."""
    _need_gpu()
    eng = _case("ns2d_mini")[2]
    ds = 3
    ngroup = ds + 2
    try:
        _options(eng, decode_group=1, decode_streams=ds)
        _check("ns2d_mini", 12, [0, 2, 3, 7, 8, 11], twice=True)
        steps = 2 * ngroup + 4
        keep2 = [t for t in range(steps) if t not in (1, 5, 6)]
        assert len(keep2) == 2 * ngroup + 1
        _check("ns2d_mini", steps, keep2, twice=True)
    finally:
        _options(eng)


@pytest.mark.parametrize("dg", [1, 2])
def test_workspace_is_the_documented_sum(dg):
    _need_gpu()
    from lns_amd import _lib
    args, model, eng, xd, z, pd, _ = _case("ns2d_mini")
    L, h = eng._L, eng._h
    N = B * M
    try:
        _options(eng, decode_group=dg)
        n0, n1, n2 = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
        assert L.lns_prepare(h, N, ctypes.byref(n0)) == 0
        assert L.lns_rollout_ensemble_workspace_bytes(h, B, M, ctypes.byref(n1)) == 0
        assert L.lns_prepare(h, N, ctypes.byref(n2)) == 0 and n2.value == n0.value

        def up(v):
            return (v + 255) // 256 * 256
        c, hh, ww = eng.latent_shape()
        xper = args.in_channels * args.Ly * args.Lx
        # include/lns.h: the lns_prepare(N) layout, two latent buffers for N, decode_streams frame buffers of decode_group steps
        assert n1.value == up(n0.value) + 2 * up(N * c * hh * ww * 4) + DEFAULTS["decode_streams"] * up(dg * N * xper * 4)
        keep = (ctypes.c_int * 3)(1, 4, 6)
        mean = torch.full((B, 3, args.in_channels, args.Ly, args.Lx), SENTINEL, device="cuda")
        var = torch.full_like(mean, SENTINEL)
        ws = torch.empty(n1.value, dtype=torch.uint8, device="cuda")
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

        def run(nbytes):
            return L.lns_rollout_latent_ensemble(h, z.data_ptr(), None, B, M, T, keep, 3, mean.data_ptr(), var.data_ptr(), None,
                                                 ws.data_ptr(), nbytes, stream)
        assert run(n1.value - 1) == _lib.LNS_ENOMEM and "ensemble workspace too small" in L.lns_last_error(h).decode()
        torch.cuda.synchronize()
        assert bool((mean == SENTINEL).all()) and bool((var == SENTINEL).all())     # nothing was enqueued
        assert run(n1.value) == 0
        torch.cuda.synchronize()
        _, mean_ref, var_ref, _ = _ref("ns2d_mini", T)
        _options(eng, decode_group=dg)
        assert _same(mean, mean_ref[:, [1, 4, 6]]) and _same(var, var_ref[:, [1, 4, 6]])
        assert L.lns_prepare(h, N, ctypes.byref(n2)) == 0 and n2.value == n0.value
    finally:
        _options(eng)


def test_check_finite_and_diagnostic_modes_after_an_ensemble_rollout():
    _need_gpu()
    args, model, eng, xd, z, pd, _ = _case("ns2d_mini")
    _ref("ns2d_mini", T)
    keep = [1, 4, 6]
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


@pytest.mark.parametrize("case", ["ns2d_mini", "twophase_cond"])
def test_predict_ensemble_is_the_hand_written_composition(case):
    """x_to_z, randn with the same generator state, rollout_latent_ensemble: equal bits; reproducible with the generator
    reset; member 0 is z0 under control=True (one member under control is predict itself)."""
    _need_gpu()
    args, model, eng, xd, z, pd, _ = _case(case)
    _options(eng)
    members, keep = 4, [0, 3, 6]
    extra = (pd[:, 0].contiguous(),) if pd is not None else ()          # [B]: shared by a trajectory's members
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    mean, var = model.predict_ensemble(xd, T, *extra, members, NOISE, generator=g, keep_steps=keep)
    g.manual_seed(5)
    z0 = model.x_to_z(xd)
    eps = torch.randn((B, members) + tuple(z0.shape[1:]), device=z0.device, generator=g) * NOISE
    zz = z0[:, None] + eps
    zz[:, 0] = z0
    param = extra[0][:, None].expand(B, members).contiguous() if extra else None
    mean_h, var_h = eng.rollout_latent_ensemble(zz, T, param=param, keep_steps=keep)
    g.manual_seed(5)
    mean_2, var_2 = model.predict_ensemble(xd, T, *extra, members, NOISE, generator=g, keep_steps=keep)
    free = model.predict_ensemble(xd, T, *extra, members, NOISE, generator=g, control=False, keep_steps=keep, return_var=False)
    one = model.predict_ensemble(xd, T, *extra, 1, NOISE, generator=g, keep_steps=keep, return_var=False)
    sel = model.predict(xd, T, *extra, to_x=True, keep_steps=keep)
    torch.cuda.synchronize()
    assert _same(mean, mean_h) and _same(var, var_h) and _same(mean, mean_2) and _same(var, var_2)
    assert not _same(free, mean) and _same(one, sel)
    assert bool((var > 0).any()) and bool(torch.isfinite(var).all())

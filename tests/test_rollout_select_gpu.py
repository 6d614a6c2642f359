"""GPU (-m gpu): the selected-step rollout (lns_rollout_select / lns_rollout_latent_select, include/lns.h; `keep_steps`
of Engine.rollout / rollout_latent / LatentDynamics.predict) against the full rollout it replaces, BIT FOR BIT.

Why equality and not a tolerance: selection adds no arithmetic.  The latent chain runs the same propagator plan on the
same values whichever buffer a step's latent lands in, and a kept step is decoded by the launch set of the full rollout
(a trajectory-step's arithmetic does not depend on the batch B * k it rides in), aimed at another slot of `out`."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from helpers import load_golden, case_args, case_inputs, rel_l2  # noqa: E402

pytestmark = pytest.mark.gpu

B, T = 3, 7                     # an odd batch: a B / T stride mix-up cannot cancel
KEEP_SETS = ([0], [6], [1, 4, 6], [0, 1, 2, 3, 4, 5, 6], [2, 3])
DEFAULTS = dict(decode_group=1, decode_streams=3, overlap=1)
ROLLOUT_TOL = 1e-4              # tests/test_gpu_parity.py: decoded fields and latents of a rollout against the reference

_cases = {}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _case(name):
    """(args, model, engine, x, param, {T: (full decoded rollout, latents)}) -- built once per preset; the full rollouts are
    the reference of every test of that preset and are never written."""
    if name not in _cases:
        import gpu_checks as gc
        from lns_amd import filler
        meta, _ = load_golden(name)
        args = case_args(meta)
        model, _ = gc.build_models(args, meta["weight_seed"])
        seed = meta["input_seed"]
        xd = torch.from_numpy(filler.normal("x", (B, args.in_channels, args.Ly, args.Lx), seed)).cuda()
        pd = torch.from_numpy(filler.uniform01("param", B, seed).astype(np.float32)).cuda() if args.family == "twophase_cond" else None
        _cases[name] = (args, model, model._engine(xd), xd, pd, {})
    return _cases[name]


def _full(name, steps):
    args, model, eng, xd, pd, refs = _case(name)
    if steps not in refs:
        _options(eng)
        full, lat = eng.rollout(xd, steps, param=pd, return_latents=True)
        torch.cuda.synchronize()
        refs[steps] = (full, lat)
    return refs[steps]


def _options(eng, **kw):
    for k, v in dict(DEFAULTS, **kw).items():
        if eng.options.get(k, DEFAULTS[k]) != v:
            eng.set_option(k, v)


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _check_keep(name, steps, keep, twice=False):
    args, model, eng, xd, pd, _ = _case(name)
    full, lat = _full(name, steps)
    ref = full[:, keep].contiguous()
    for _ in range(2 if twice else 1):
        sel, sel_lat = eng.rollout(xd, steps, param=pd, keep_steps=keep, return_latents=True)
        torch.cuda.synchronize()
        assert sel.shape == (B, len(keep), args.in_channels, args.Ly, args.Lx)
        assert _same(sel, ref), (name, keep, eng.options)
        assert _same(sel_lat, lat), (name, keep, eng.options)


GRID = [("ns2d_mini", dg, ds, ov) for dg in (1, 2, 3, 0) for ds in (1, 3) for ov in (0, 1)] + \
       [(c, dg, ds, 1) for c in ("twophase_cond", "sw_half_periodic") for dg in (1, 2) for ds in (1, 3)]


@pytest.mark.parametrize("case,dg,ds,ov", GRID)
def test_selected_steps_have_the_bits_of_the_full_rollout(case, dg, ds, ov):
    """out[:, i] == full[:, keep[i]] and latents_out == the full call's, for every scheduling option: decode_group = 3 with
    five and seven kept steps has a ragged last group, decode_group = 2 with [1, 4, 6] a group of steps that are not consecutive,
    [2, 3] ends in a run of skipped steps."""
    _need_gpu()
    eng = _case(case)[2]
    _full(case, T)
    try:
        _options(eng, decode_group=dg, decode_streams=ds, overlap=ov)
        for keep in KEEP_SETS:
            _check_keep(case, T, keep)
        _check_keep(case, T, [0, 2, 3, 4, 6])                     # five kept steps: 3 + 2 at decode_group = 3
    finally:
        _options(eng)


def test_ring_groups_are_reused_under_selection():
    """More kept groups than ring groups: the chain's write-after-read wait guards a group that was filled many chain steps
    earlier.  The ring holds decode_streams + 2 groups (csrc/lns_engine.cpp ws_layout: one being written, one per decode
    stream, one spare); the second keep set is the smallest that wraps it twice (2 * ngroup + 1 groups of one step), with
    skipped steps in between.  Twice in a row on the same workspace."""
    _need_gpu()
    args, model, eng, xd, pd, _ = _case("ns2d_mini")
    ds = 3
    ngroup = ds + 2
    try:
        _options(eng, decode_group=1, decode_streams=ds)
        keep = [0, 2, 3, 7, 8, 11]
        assert len(keep) > ngroup
        _check_keep("ns2d_mini", 12, keep, twice=True)
        steps = 2 * ngroup + 4
        keep2 = [t for t in range(steps) if t not in (1, 5, 6)]
        assert len(keep2) == 2 * ngroup + 1
        _check_keep("ns2d_mini", steps, keep2, twice=True)
    finally:
        _options(eng)


@pytest.mark.parametrize("case", ["ns2d_mini", "twophase_cond"])
def test_rollout_latent_select_and_chunks(case):
    _need_gpu()
    args, model, eng, xd, pd, _ = _case(case)
    full, lat = _full(case, T)
    _options(eng)
    keep = [1, 4, 6]
    z0 = eng.encode(xd, pd) if eng.cfg.cond_encoder else eng.encode(xd)
    sel = eng.rollout(xd, T, param=pd, keep_steps=keep)
    lsel, z_last = eng.rollout_latent(z0, T, param=pd, keep_steps=keep)
    torch.cuda.synchronize()
    assert _same(lsel, sel) and _same(sel, full[:, keep].contiguous())
    assert _same(z_last, lat[:, -1].contiguous())
    # two chained chunks, kept steps in both; the first ends in skipped steps (its z_last comes out of a ping-pong buffer)
    a, z4 = eng.rollout_latent(z0, 4, param=pd, keep_steps=[1])
    b, z7 = eng.rollout_latent(z4, 3, param=pd, keep_steps=[0, 2])
    torch.cuda.synchronize()
    assert _same(z4, lat[:, 3].contiguous()) and _same(z7, z_last)
    assert _same(torch.cat([a, b], 1), sel)
    # a preallocated output
    out = torch.full_like(sel, float("nan"))
    assert eng.rollout(xd, T, param=pd, keep_steps=range(1, 7, 3), out=out[:, :2].contiguous()).shape[1] == 2
    assert eng.rollout(xd, T, param=pd, keep_steps=keep, out=out) is out and _same(out, sel)


@pytest.mark.parametrize("case", ["ns2d_mini", "twophase_cond", "sw_half_periodic"])
def test_kept_steps_match_reference_golden(case):
    """The stored steps of the golden fixture (the REAL reference's decoded rollout and latents), decoded on their own:
    tolerance and helper of test_gpu_parity.py::test_rollout_matches_reference_golden (selection adds no arithmetic)."""
    _need_gpu()
    model = _case(case)[1]
    meta, g = load_golden(case)
    args = case_args(meta)
    x, param = case_inputs(meta, args)
    xd = torch.from_numpy(x).cuda()
    extra = (torch.from_numpy(param).cuda(),) if param is not None else ()
    _options(model._engine(xd))
    keep = [s - 1 for s in meta["steps"]]
    dec, lat = model.predict(xd, meta["T"], *extra, to_x=True, return_latents=True, keep_steps=keep)
    torch.cuda.synchronize()
    dec, lat = dec.cpu().numpy(), lat.cpu().numpy()
    assert dec.shape == (meta["B"], len(keep), args.in_channels, args.Ly, args.Lx) and lat.shape[1] == meta["T"]
    sub = meta["sub"]
    report = []
    for i, s in enumerate(meta["steps"]):
        e_lat = rel_l2(lat[:, s - 1], g["lat"][:, i])
        e_dec = rel_l2(dec[:, i][..., ::sub, ::sub], g["dec"][:, i])
        report.append((s, e_lat, e_dec))
        assert e_dec < ROLLOUT_TOL and e_lat < ROLLOUT_TOL, report
    print(case, report)


def test_refusals_on_the_device_build():
    _need_gpu()
    from lns_amd import _lib
    from lns_amd._lib import LnsError
    args, model, eng, xd, pd, _ = _case("ns2d_mini")
    _options(eng)
    L, h = eng._L, eng._h
    n0, n1, n2 = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert L.lns_prepare(h, B, ctypes.byref(n0)) == 0
    assert L.lns_rollout_select_workspace_bytes(h, B, ctypes.byref(n1)) == 0
    assert L.lns_prepare(h, B, ctypes.byref(n2)) == 0 and n2.value == n0.value

    def up(v):
        return (v + 255) // 256 * 256
    c, hh, ww = eng.latent_shape()
    # include/lns.h: the lns_prepare layout, then two latent buffers of B * c * h * w floats, each rounded up to 256 bytes
    assert n1.value - up(n0.value) == 2 * up(B * c * hh * ww * 4) > 0
    keep = (ctypes.c_int * 3)(1, 4, 6)
    SENTINEL = -12345.0
    out = torch.full((B, 3, args.in_channels, args.Ly, args.Lx), SENTINEL, device="cuda")
    ws = torch.empty(n1.value, dtype=torch.uint8, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run(nbytes, k=keep, nk=3):
        return L.lns_rollout_select(h, xd.data_ptr(), None, B, T, k, nk, out.data_ptr(), None, ws.data_ptr(), nbytes, stream)
    assert run(n1.value - 1) == _lib.LNS_ENOMEM and "workspace" in L.lns_last_error(h).decode()
    assert run(n0.value) == _lib.LNS_ENOMEM                      # the rollout's own workspace is not enough
    assert run(n1.value, k=(ctypes.c_int * 3)(1, 6, 4)) == _lib.LNS_EINVAL and "keep_steps" in L.lns_last_error(h).decode()
    assert run(n1.value, nk=0) == _lib.LNS_EINVAL
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())                         # a refused call touches nothing
    assert run(n1.value) == 0
    torch.cuda.synchronize()
    assert _same(out, _full("ns2d_mini", T)[0][:, [1, 4, 6]].contiguous())
    with pytest.raises(LnsError, match="slice the latent rollout"):
        eng.rollout(xd, T, to_x=False, keep_steps=[1, 4])
    with pytest.raises(LnsError, match="slice the latent rollout"):
        model.predict(xd, T, keep_steps=[1, 4])                  # predict's default is to_x=False
    with pytest.raises(LnsError, match="keep_steps"):
        eng.rollout(xd, T, keep_steps=[4, 1])
    with pytest.raises(LnsError, match="preallocated"):
        eng.rollout(xd, T, keep_steps=[1, 4], out=out)


def test_no_existing_behaviour_moved():
    """predict(x, T, to_x=True) before and after a selected call on the same model: equal bits; lns_prepare's size is
    what it was; the rollout still runs in exactly lns_prepare's bytes."""
    _need_gpu()
    from lns_amd import _lib
    args, model, eng, xd, pd, _ = _case("ns2d_mini")
    _options(eng)
    L, h = eng._L, eng._h
    n0, n1 = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert L.lns_prepare(h, B, ctypes.byref(n0)) == 0
    before = model.predict(xd, T, to_x=True).clone()
    lat_before = model.predict(xd, T).clone()
    sel = model.predict(xd, T, to_x=True, keep_steps=slice(None, None, 3))
    after = model.predict(xd, T, to_x=True)
    lat_after = model.predict(xd, T)
    torch.cuda.synchronize()
    assert _same(before, after) and _same(lat_before, lat_after) and _same(before, _full("ns2d_mini", T)[0])
    assert _same(sel, before[:, ::3].contiguous()) and sel.shape[1] == 3
    assert L.lns_prepare(h, B, ctypes.byref(n1)) == 0 and n1.value == n0.value
    small = torch.empty(n0.value, dtype=torch.uint8, device="cuda")
    out = torch.empty_like(before)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.lns_rollout(h, xd.data_ptr(), None, B, T, 1, out.data_ptr(), None, small.data_ptr(), n0.value, stream) == 0
    assert L.lns_rollout(h, xd.data_ptr(), None, B, T, 1, out.data_ptr(), None, small.data_ptr(), n0.value - 1, stream) == _lib.LNS_ENOMEM
    torch.cuda.synchronize()
    assert _same(out, before)


def test_check_finite_and_diagnostic_modes_after_a_selected_rollout():
    _need_gpu()
    args, model, eng, xd, pd, _ = _case("ns2d_mini")
    full = _full("ns2d_mini", T)[0]
    keep = [1, 4, 6]
    ref = full[:, keep].contiguous()
    try:
        for opts in (dict(), dict(decode_group=2), dict(overlap=0)):
            _options(eng, **opts)
            sel = eng.rollout(xd, T, keep_steps=keep)
            eng.check_finite(B, xd.device)                       # LNS_OK: raises otherwise
            assert _same(sel, ref)
        _options(eng, decode_group=2)
        eng.set_option("track_nonfinite", 1)
        sel = eng.rollout(xd, T, keep_steps=keep)
        eng.check_finite(B)
        assert _same(sel, ref)
        eng.set_option("track_nonfinite", 0)
        eng.timing_enable(True)                                  # diagnostics mode: everything on the caller's stream
        sel = eng.rollout(xd, T, keep_steps=keep)
        torch.cuda.synchronize()
        eng.timing_enable(False)
        assert _same(sel, ref)
    finally:
        eng.timing_enable(False)
        eng.set_option("track_nonfinite", 0)
        _options(eng)

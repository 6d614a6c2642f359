"""CPU: the flow diagnostics (include/lns.h "flow diagnostics"; lns_rollout_eval_flow, lns_op_flow_stats, lns_op_vorticity).

The licence of tests/flow_stats_reference.py: its float64 form against numpy.gradient, a rolled central difference and two
flows with known answers (Taylor-Green, solid-body rotation), and four deliberate mistakes that it must tell from the
statement.  Then what needs no device: the symbols, lns_build_has, the refusal matrix of the three kinds of entry point
(code, message, order) and boundary="auto" per preset."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import flow_stats_reference as fl  # noqa: E402
from helpers import ROOT  # noqa: E402

FLOW_SYMBOLS = ("lns_rollout_eval_flow", "lns_rollout_latent_eval_flow", "lns_op_flow_stats", "lns_op_vorticity")
COL = {n: i for i, n in enumerate(fl.NAMES)}


# ---- the reference's licence, in float64 ------------------------------------------------------------------------------
def test_derivative_is_numpy_gradient_on_walls_and_a_rolled_difference_on_periodic_axes():
    rng = np.random.default_rng(3)
    for H, W in ((2, 2), (3, 5), (17, 16), (2, 9)):
        f = rng.standard_normal((2, 1, H, W))
        t = torch.from_numpy(f)
        for d in (0.25, 0.5, 0.3):
            d32 = float(np.float32(d))
            for dim, axis in ((-2, 2), (-1, 3)):
                got = fl.deriv(t, dim, True, d, torch.float64).numpy()
                assert np.allclose(got, np.gradient(f, d32, axis=axis, edge_order=1), rtol=1e-14, atol=1e-14), (H, W, d, dim)
                got = fl.deriv(t, dim, False, d, torch.float64).numpy()
                want = (np.roll(f, -1, axis) - np.roll(f, 1, axis)) / (2.0 * d32)
                assert np.allclose(got, want, rtol=1e-14, atol=1e-14), (H, W, d, dim)
    one = torch.from_numpy(rng.standard_normal((1, 1, 1, 7)))
    assert bool((fl.deriv(one, -2, True, 0.5, torch.float64) == 0).all()) and bool((fl.deriv(one, -2, False, 0.5, torch.float64) == 0).all())


def _as_fields(u, v):
    """u, v [H, W] float64 -> [1, 1, 2, H, W] float64 (the float64 references take float64 inputs as they are)."""
    return torch.from_numpy(np.stack([u, v])[None, None])


def test_taylor_green_is_divergence_free_with_known_energy_and_enstrophy():
    """u = sin x cos y, v = -cos x sin y on a periodic N x N grid, h = 2 pi / N.  The central differences give
    dv = 0 and w = 2 sin x sin y sin(h) / d for any divisor d; the reference divides by the fp32 spacing d = (float)h."""
    N = 64
    h = 2.0 * math.pi / N
    d = float(np.float32(h))
    x = (np.arange(N) * h)[None, :]
    y = (np.arange(N) * h)[:, None]
    f = _as_fields(np.sin(x) * np.cos(y), -np.cos(x) * np.sin(y))
    bc = (fl.PERIODIC, fl.PERIODIC)
    U, V, w, dv = fl.pixel_fields(f, 0, 1, h, h, bc, {}, torch.float64)
    grad = fl.deriv(U, -1, False, h, torch.float64)
    assert float(dv.abs().max()) < 1e-14 * float(grad.abs().max())
    assert np.allclose(w[0, 0].numpy(), 2.0 * np.sin(x) * np.sin(y) * math.sin(h) / d, rtol=0, atol=1e-13)
    s = fl.stats64(f, f, dx=h, dy=h, bc=bc)[0, 0]
    assert abs(float(s[COL["ke_P"]]) - 0.25) < 1e-14 and abs(float(s[COL["ke_Q"]]) - 0.25) < 1e-14
    want = (math.sin(h) / d) ** 2 / 2.0
    assert abs(float(s[COL["ens_P"]]) - want) < 1e-13 * want and abs(float(s[COL["ens_Q"]]) - want) < 1e-13 * want
    assert float(s[COL["div_P"]]) < 1e-14 * float(grad.abs().max())
    assert float(s[COL["vort_err"]]) == 0 and float(s[COL["vel_err"]]) == 0 and abs(float(s[COL["vort_cos"]]) - 1) < 1e-7


def test_solid_body_rotation_with_walls():
    H, W = 9, 13
    d = 0.5
    x = (np.arange(W) * d)[None, :] + 0 * np.arange(H)[:, None]
    y = (np.arange(H) * d)[:, None] + 0 * np.arange(W)[None, :]
    f = _as_fields(-y, x)
    U, V, w, dv = fl.pixel_fields(f, 0, 1, d, d, (fl.WALL, fl.WALL), {}, torch.float64)
    assert bool((w == 2.0).all()) and bool((dv == 0.0).all())          # edges included
    w32 = fl.vorticity32(f, dx=d, dy=d, bc=(fl.WALL, fl.WALL))
    assert bool((w32 == 2.0).all())
    s = fl.stats64(f, f, dx=d, dy=d, bc=(fl.WALL, fl.WALL))[0, 0]
    assert float(s[COL["ens_P"]]) == 2.0 and float(s[COL["div_P"]]) == 0.0 and float(s[COL["maxvort_Q"]]) == 2.0


# ---- deliberate mistakes ----------------------------------------------------------------------------------------------
MISTAKE_PLANES = ((3, 5), (17, 16), (61, 121))
DX, DY = 0.25, 0.5


def _moved(wrong, right):
    """The largest relative move of a column: max |wrong - right| / max |right| per column."""
    d = (wrong - right).abs().reshape(-1, wrong.shape[-1]).amax(0)
    return float((d / right.abs().reshape(-1, right.shape[-1]).amax(0)).max())


def _sign_mistake(y_hat, bc):
    """ens_P and maxvort_P with w = dxV + dyU."""
    D = fl.denorm(y_hat, {}, torch.float64)
    U, V = D[:, :, 0], D[:, :, 1]
    w = fl.deriv(V, -1, bc[1] == fl.WALL, DX, torch.float64) + fl.deriv(U, -2, bc[0] == fl.WALL, DY, torch.float64)
    return torch.stack([0.5 * (w * w).mean((-2, -1)), w.abs().amax((-2, -1))], -1)


@pytest.mark.parametrize("plane", MISTAKE_PLANES, ids=lambda p: "%dx%d" % p)
def test_the_reference_tells_four_mistakes_from_the_statement(plane):
    """u / v swapped, the sign of dyU, dx / dy swapped, the two boundary codes swapped: each moves some column by at least
    6e-2 relative, more than 100 x the bound max(2e-7, 3 x own) the kernel is held to (test_eval_flow_gpu.py)."""
    g = torch.Generator().manual_seed(100 * plane[0] + plane[1])
    y = torch.randn((2, 2, 3) + plane, generator=g)
    y_hat = y + 0.3 * torch.randn(y.shape, generator=g)
    for bc in ((fl.WALL, fl.PERIODIC), (fl.PERIODIC, fl.PERIODIC), (fl.WALL, fl.WALL)):
        right = fl.stats64(y_hat, y, dx=DX, dy=DY, bc=bc)
        moves = {
            "uv_swapped": _moved(fl.stats64(y_hat, y, u=1, v=0, dx=DX, dy=DY, bc=bc), right),
            "dx_dy_swapped": _moved(fl.stats64(y_hat, y, dx=DY, dy=DX, bc=bc), right),
            "sign_of_dyU": _moved(_sign_mistake(y_hat, bc), right[..., [COL["ens_P"], COL["maxvort_P"]]]),
        }
        if bc[0] != bc[1]:                                                # the swap shows only with mixed boundaries
            moves["boundaries_swapped"] = _moved(fl.stats64(y_hat, y, dx=DX, dy=DY, bc=bc[::-1]), right)
        print(plane, bc, {k: "%.3e" % m for k, m in moves.items()})
        for name, m in moves.items():
            assert m >= 6e-2, (plane, bc, name, m)


# ---- the library: symbols, feature, refusals ----------------------------------------------------------------------------
def test_flow_symbols_are_declared_exported_and_bound():
    from lns_amd import _lib
    _lib.build()
    src = open(os.path.join(ROOT, "include", "lns.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(lns_[a-z0-9_]+)\s*\(", src))
    L = ctypes.CDLL(_lib.LIB_PATH)
    for s in FLOW_SYMBOLS:
        assert s in declared, "not declared in include/lns.h: " + s
        assert hasattr(L, s), "missing export: " + s
        assert s in _lib.SYMBOLS
        assert getattr(_lib.lib(), s).argtypes, "not bound in _lib.lib(): " + s
    assert re.search(r"#define\s+LNS_ABI_VERSION\s+2\b", src)            # additive: the ABI version stays
    assert re.search(r"#define\s+LNS_FLOW_STATS\s+12\b", src) and _lib.LNS_FLOW_STATS == 12
    from lns_amd import metrics
    assert metrics.FLOW_STATS == fl.NAMES


def test_build_has_eval_flow():
    from lns_amd import _lib
    assert _lib.lib().lns_build_has(b"eval_flow") == 1


def test_struct_mirrors_have_the_header_layout():
    """lns_flow_spec: ten 4-byte members; lns_eval_flow: two 4-byte members and five pointers."""
    from lns_amd import _lib
    assert ctypes.sizeof(_lib.LnsFlowSpec) == 40
    assert ctypes.sizeof(_lib.LnsEvalFlow) == 8 + 5 * ctypes.sizeof(ctypes.c_void_p)
    assert _lib.LnsFlowSpec.dy.offset == 20 and _lib.LnsFlowSpec.dx.offset == 24 and _lib.LnsFlowSpec.nbins.offset == 28


_T = 5
_P = ctypes.c_void_p(0x1000)                          # stands for a device pointer; never dereferenced


def _ints(*v):
    return (ctypes.c_int * len(v))(*v)


def _engines():
    from lns_amd import _lib, config, engine
    mini = config.preset("ns2d_mini")
    mk = lambda a, **kw: engine.Engine(engine.make_config(a, ae_prefix="vq_ae.", prop_prefix="propagator.", **kw))
    engines = {"full": mk(mini), "max4": mk(mini), "noprop": mk(mini, prop_kind=_lib.LNS_PROP_NONE)}
    engines["max4"].set_option("eval_max_steps", 4)
    return engines


def _fspec(**kw):
    from lns_amd import engine
    fs = engine.flow_spec(0, 1, 0.25, 0.5, ("wall", "periodic"), (8, -2.0, 2.0))
    for k, val in kw.items():
        setattr(fs, k, val)
    return fs


def _rollout_call(L, engines, entry, kw):
    """-> (rc, message) of one lns_rollout_eval_flow / lns_rollout_latent_eval_flow call on fake device pointers."""
    from lns_amd import _lib, engine
    a = dict(eng="full", start=_P, y=_P, B=3, T=_T, spec="ok", frame=_P, k=_ints(0, 3, 4), nk=3, frames=_P, sel=None,
             flow="ok", fspec=_fspec(), flow_out=_P, n_flow=2, steps=_ints(1, 4), hist=_P, vort=_P)
    a.update(kw)
    e = engines[a["eng"]]
    spec = engine.eval_spec(2, mean=0.37, std=1.9)
    if a["spec"] == "bad":
        spec.size = 8
    sp = ctypes.byref(spec) if a["spec"] else None
    q = None
    if a["sel"] is not None:
        q = _lib.LnsEvalSelect()
        q.size = ctypes.sizeof(_lib.LnsEvalSelect)
        for k, val in a["sel"].items():
            setattr(q, k, val)
    f = None
    if a["flow"]:
        f = _lib.LnsEvalFlow()
        f.size = ctypes.sizeof(_lib.LnsEvalFlow) if a["flow"] == "ok" else 8
        f.n_flow, f.flow_steps_host = a["n_flow"], a["steps"]
        if a["fspec"] is not None:
            f.fspec = ctypes.pointer(a["fspec"])
        f.flow_out, f.hist_out, f.vort_frames_out = a["flow_out"], a["hist"], a["vort"]
    head = (e._h, a["start"], None, a["y"], a["B"], a["T"])
    tail = (_P, 1 << 40, None, ctypes.byref(q) if q is not None else None, ctypes.byref(f) if f is not None else None)
    if entry == "lns_rollout_eval_flow":
        rc = L.lns_rollout_eval_flow(*head, sp, a["frame"], _P, a["k"], a["nk"], a["frames"], *tail)
    else:
        rc = L.lns_rollout_latent_eval_flow(*head, 0, a["T"], sp, a["frame"], _P, a["k"], a["nk"], a["frames"], None, *tail)
    return rc, L.lns_last_error(e._h).decode()


_NOT_FINAL = "lns_finalize_weights must be called first"      # what stops a call that passes every refusal here: no weights
_KEEP_MSG = "keep_steps must be ascending steps in [0, 5): entry 2 is 3"
_FLOW_NULL = "flow is null or its size field is not sizeof(lns_eval_flow)"
_FSPEC_NULL = "fspec is null or its size field is not sizeof(lns_flow_spec)"
_CHANNELS = "fspec: cu and cv must be two different channels of the fields"
_BC = "fspec: bc_y and bc_x must be LNS_FLOW_PERIODIC (0) or LNS_FLOW_WALL (1)"
_SPACING = "fspec: dx and dy must be finite and positive"
_NBINS = "fspec: nbins must be in 0 .. 256"
_EDGES = "fspec: the edges must be finite with hi > lo"
_HIST = "hist_out needs fspec->nbins > 0"
_VORT = "vort_frames_out needs n_keep > 0"
_MAPS = "sel asks for time maps: the flow form keeps the workspace of lns_rollout_eval (lns_rollout_eval_maps has them)"
_ROLLOUT_CASES = {
    # a call that passes every refusal is stopped by the missing weights: nothing touched the device
    "valid": (dict(), (-3, _NOT_FINAL)),
    "valid_without_options": (dict(hist=None, vort=None, nk=0, k=None, frames=None, fspec=_fspec(nbins=0)), (-3, _NOT_FINAL)),
    "valid_with_selections": (dict(sel=dict(n_stats=1, stats_steps_host=_ints(2), stats_out=0x1000, n_spec=1, spectrum_steps_host=_ints(0),
                                            spectra_out=0x1000)), (-3, _NOT_FINAL)),
    # lns_rollout_eval's
    "start_null": (dict(start=None), (-1, None)), "y_null": (dict(y=None), (-1, "y_true is null")),
    "spec_bad": (dict(spec="bad"), (-1, "spec is null or its size field is not sizeof(lns_eval_spec)")),
    "keep_unsorted": (dict(k=_ints(0, 4, 3)), (-1, _KEEP_MSG)),
    # the selections'
    "stats_out_null": (dict(sel=dict(n_stats=1, stats_steps_host=_ints(2))), (-1, "stats_out is null")),
    "spectrum_steps_bad": (dict(sel=dict(n_spec=1, spectrum_steps_host=_ints(5), spectra_out=0x1000)),
                           (-1, "spectrum_steps must be ascending steps in [0, 5): entry 0 is 5")),
    "sel_wrong_size": (dict(sel=dict(size=8)), (-1, "sel: the size field is not sizeof(lns_eval_select)")),
    "sel_maps_out": (dict(sel=dict(maps_out=0x1000)), (-1, _MAPS)), "sel_map_every": (dict(sel=dict(map_every=1)), (-1, _MAPS)),
    # the flow part, in the order of include/lns.h
    "flow_null": (dict(flow=None), (-1, _FLOW_NULL)), "flow_wrong_size": (dict(flow="bad"), (-1, _FLOW_NULL)),
    "flow_out_null": (dict(flow_out=None), (-1, "flow_out is null")),
    "n_flow_0": (dict(n_flow=0), (-1, "n_flow must be at least 1")), "n_flow_negative": (dict(n_flow=-1), (-1, "n_flow must be at least 1")),
    "steps_null": (dict(steps=None), (-1, "flow_steps is null")),
    "steps_T": (dict(steps=_ints(1, 5)), (-1, "flow_steps must be ascending steps in [0, 5): entry 1 is 5")),
    "steps_negative": (dict(steps=_ints(-1, 2)), (-1, "flow_steps must be ascending steps in [0, 5): entry 0 is -1")),
    "steps_not_ascending": (dict(steps=_ints(2, 2)), (-1, "flow_steps must be ascending steps in [0, 5): entry 1 is 2")),
    "fspec_null": (dict(fspec=None), (-1, _FSPEC_NULL)), "fspec_wrong_size": (dict(fspec=_fspec(size=36)), (-1, _FSPEC_NULL)),
    "cu_equals_cv": (dict(fspec=_fspec(cv=0)), (-1, _CHANNELS)), "cu_negative": (dict(fspec=_fspec(cu=-1)), (-1, _CHANNELS)),
    "cv_past_channels": (dict(fspec=_fspec(cv=2)), (-1, _CHANNELS)),
    "bc_y_2": (dict(fspec=_fspec(bc_y=2)), (-1, _BC)), "bc_x_negative": (dict(fspec=_fspec(bc_x=-1)), (-1, _BC)),
    "dx_0": (dict(fspec=_fspec(dx=0.0)), (-1, _SPACING)), "dy_negative": (dict(fspec=_fspec(dy=-0.5)), (-1, _SPACING)),
    "dx_inf": (dict(fspec=_fspec(dx=float("inf"))), (-1, _SPACING)), "dy_nan": (dict(fspec=_fspec(dy=float("nan"))), (-1, _SPACING)),
    "nbins_negative": (dict(fspec=_fspec(nbins=-1)), (-1, _NBINS)), "nbins_257": (dict(fspec=_fspec(nbins=257)), (-1, _NBINS)),
    "edges_equal": (dict(fspec=_fspec(hi=-2.0)), (-1, _EDGES)), "edge_nan": (dict(fspec=_fspec(lo=float("nan"))), (-1, _EDGES)),
    "edge_inf": (dict(fspec=_fspec(hi=float("inf"))), (-1, _EDGES)),
    "edges_unused_without_bins": (dict(fspec=_fspec(nbins=0, hi=-9.0), hist=None), (-3, _NOT_FINAL)),
    "hist_without_bins": (dict(fspec=_fspec(nbins=0)), (-1, _HIST)),
    "vort_without_keep": (dict(nk=0, k=None, frames=None), (-1, _VORT)),
    # the rest of lns_rollout_eval's
    "B_huge": (dict(B=1 << 30), (-1, None)),
    "past_eval_max_steps": (dict(eng="max4"), (-1, "5 steps exceed the option eval_max_steps = 4 (it sizes the evaluation workspace)")),
    "no_propagator": (dict(eng="noprop"), (-3, "rollout needs autoencoder and propagator")),
    # which of two failing checks answers
    "flow_null+keep_unsorted": (dict(flow=None, k=_ints(0, 4, 3)), (-1, _KEEP_MSG)),
    "flow_null+stats_out_null": (dict(flow=None, sel=dict(n_stats=1, stats_steps_host=_ints(2))), (-1, "stats_out is null")),
    "flow_null+sel_maps_out": (dict(flow=None, sel=dict(maps_out=0x1000)), (-1, _MAPS)),
    "sel_wrong_size+sel_maps": (dict(sel=dict(size=8, maps_out=0x1000)), (-1, "sel: the size field is not sizeof(lns_eval_select)")),
    "flow_out_null+n_flow_0": (dict(flow_out=None, n_flow=0), (-1, "flow_out is null")),
    "n_flow_0+steps_null": (dict(n_flow=0, steps=None), (-1, "n_flow must be at least 1")),
    "steps_null+fspec_null": (dict(steps=None, fspec=None), (-1, "flow_steps is null")),
    "steps_T+fspec_null": (dict(steps=_ints(1, 5), fspec=None), (-1, "flow_steps must be ascending steps in [0, 5): entry 1 is 5")),
    "cu_equals_cv+bc": (dict(fspec=_fspec(cv=0, bc_y=3)), (-1, _CHANNELS)), "bc+dx": (dict(fspec=_fspec(bc_y=3, dx=0.0)), (-1, _BC)),
    "dx+nbins": (dict(fspec=_fspec(dx=0.0, nbins=300)), (-1, _SPACING)), "nbins+vort": (dict(fspec=_fspec(nbins=300), nk=0, k=None, frames=None), (-1, _NBINS)),
    "edges+vort": (dict(fspec=_fspec(hi=-3.0), nk=0, k=None, frames=None), (-1, _EDGES)),
    "hist+vort": (dict(fspec=_fspec(nbins=0), nk=0, k=None, frames=None), (-1, _HIST)),
    "vort+B_huge": (dict(nk=0, k=None, frames=None, B=1 << 30), (-1, _VORT)),
    "vort+no_propagator": (dict(nk=0, k=None, frames=None, eng="noprop"), (-1, _VORT)),
}


@pytest.mark.parametrize("entry", ["lns_rollout_eval_flow", "lns_rollout_latent_eval_flow"])
def test_rollout_entry_points_refuse_in_the_documented_order_without_a_device(entry):
    from lns_amd import _lib
    L = _lib.lib()
    engines = _engines()
    fn = getattr(L, entry)
    assert fn(*[0 if t in (ctypes.c_int, ctypes.c_size_t) else None for t in fn.argtypes]) == _lib.LNS_EINVAL     # a null engine
    for name, (kw, (code, msg)) in _ROLLOUT_CASES.items():
        rc, got = _rollout_call(L, engines, entry, kw)
        assert rc == code, (entry, name, rc, got)
        if msg is not None:
            assert got == msg, (entry, name, got)
    # the step message of a latent chunk speaks of the chunk's T
    rc, got = _rollout_call(L, engines, entry, dict(T=3, k=_ints(0, 2), nk=2, steps=_ints(1, 3)))
    assert rc == -1 and got == "flow_steps must be ascending steps in [0, 3): entry 1 is 3"


def _op_call(L, op, kw):
    from lns_amd import engine
    a = dict(a=_P, y=_P, dims=(2, 3, 2, 4, 6), spec="ok", fspec=_fspec(), out=_P, hist=_P)
    a.update(kw)
    spec = engine.eval_spec(a["dims"][2], mean=0.37, std=1.9) if a["spec"] != "per_channel" else None
    if a["spec"] == "per_channel":                                       # the per-channel form on nine channels
        spec = engine.eval_spec(8, mean=[0.0] * 8, std=[1.0] * 8)
    if a["spec"] == "bad":
        spec.size = 8
    sp = ctypes.byref(spec) if a["spec"] else None
    fp = ctypes.byref(a["fspec"]) if a["fspec"] is not None else None
    if op == "flow_stats":
        rc = L.lns_op_flow_stats(a["a"], a["y"], *a["dims"], sp, fp, a["out"], a["hist"], None)
    else:
        rc = L.lns_op_vorticity(a["a"], *a["dims"], sp, fp, a["out"], None)
    return rc, L.lns_create_error().decode()


_SHAPE = "B, T, H, W >= 1, C >= 2, H * W <= 2^30 and B * T < 2^24"
_OP_CASES = {
    "fields_null": (dict(a=None), "is null"), "out_null": (dict(out=None), "is null"),
    "spec_null": (dict(spec=None), "spec is null or its size field is not sizeof(lns_eval_spec)"),
    "spec_bad": (dict(spec="bad"), "spec is null or its size field is not sizeof(lns_eval_spec)"),
    "T_0": (dict(dims=(2, 0, 2, 4, 6)), _SHAPE), "C_1": (dict(dims=(2, 3, 1, 4, 6)), _SHAPE), "W_0": (dict(dims=(2, 3, 2, 4, 0)), _SHAPE),
    "plane_too_large": (dict(dims=(1, 1, 2, 1 << 16, (1 << 14) + 1)), _SHAPE), "too_many_frames": (dict(dims=(1 << 12, 1 << 12, 2, 4, 6)), _SHAPE),
    "per_channel_on_9_channels": (dict(dims=(2, 3, 9, 4, 6), spec="per_channel"), "the per-channel form needs C <= 8"),
    "fspec_null": (dict(fspec=None), _FSPEC_NULL), "fspec_wrong_size": (dict(fspec=_fspec(size=44)), _FSPEC_NULL),
    "cu_equals_cv": (dict(fspec=_fspec(cu=1)), _CHANNELS), "cv_past_channels": (dict(fspec=_fspec(cv=2)), _CHANNELS),
    "bc_x_2": (dict(fspec=_fspec(bc_x=2)), _BC), "dy_0": (dict(fspec=_fspec(dy=0.0)), _SPACING), "dx_nan": (dict(fspec=_fspec(dx=float("nan"))), _SPACING),
    "nbins_257": (dict(fspec=_fspec(nbins=257)), _NBINS), "edges": (dict(fspec=_fspec(lo=2.0)), _EDGES),
    # which of two failing checks answers
    "out_null+spec_null": (dict(out=None, spec=None), "is null"), "spec_null+T_0": (dict(spec=None, dims=(2, 0, 2, 4, 6)), "spec is null"),
    "T_0+fspec_null": (dict(dims=(2, 0, 2, 4, 6), fspec=None), _SHAPE), "cv_past_channels+bc": (dict(fspec=_fspec(cv=2, bc_y=7)), _CHANNELS),
    "bc+dx": (dict(fspec=_fspec(bc_y=7, dx=-1.0)), _BC), "dx+nbins": (dict(fspec=_fspec(dx=-1.0, nbins=-3)), _SPACING),
}


@pytest.mark.parametrize("op", ["flow_stats", "vorticity"])
def test_ops_refuse_in_the_documented_order_without_a_device(op):
    from lns_amd import _lib
    L = _lib.lib()
    cases = dict(_OP_CASES)
    if op == "flow_stats":
        cases.update({"y_null": (dict(y=None), "is null"), "hist_without_bins": (dict(fspec=_fspec(nbins=0)), _HIST),
                      "edges+hist": (dict(fspec=_fspec(nbins=0, lo=9.0)), _HIST), "nbins+hist": (dict(fspec=_fspec(nbins=-1)), _NBINS)})
    for name, (kw, msg) in cases.items():
        rc, got = _op_call(L, op, kw)
        assert rc == _lib.LNS_EINVAL and got.startswith(op + ": ") and msg in got, (op, name, rc, got)


# ---- Python: boundaries, specs, wrappers ------------------------------------------------------------------------------------
def test_flow_boundary_and_auto_per_preset():
    from lns_amd import config, engine, metrics
    from lns_amd._lib import LnsError
    assert metrics.flow_boundary("periodic") == (0, 0) and metrics.flow_boundary("wall") == (1, 1)
    assert metrics.flow_boundary(("wall", "periodic")) == (1, 0) and metrics.flow_boundary(["periodic", "wall"]) == (0, 1)
    for bad in ("walls", "Periodic", 1, None, ("wall",), ("wall", "periodic", "wall"), ("wall", 0)):
        with pytest.raises(LnsError, match="flow boundary"):
            metrics.flow_boundary(bad)
    with pytest.raises(LnsError, match="needs a model"):
        metrics.flow_boundary("auto")
    x = torch.zeros((1, 1, 2, 4, 4))
    with pytest.raises(LnsError, match="needs a model"):
        metrics.flow_stats(x, x, boundary="auto")                        # the boundary is read before the tensors
    with pytest.raises(LnsError, match="no CPU fallback"):
        metrics.flow_stats(x, x)
    with pytest.raises(LnsError, match="no CPU fallback"):
        metrics.vorticity(x)
    want = {"ns2d_mini": (0, 0), "ns2d_64": (0, 0), "ns2d_128": (0, 0), "sw_half_periodic": (1, 0), "twophase": (1, 1),
            "twophase_cond": (1, 1)}
    for name, codes in want.items():
        eng = engine.Engine(engine.make_config(config.preset(name), ae_prefix="vq_ae.", prop_prefix="propagator."))
        assert metrics.flow_boundary("auto", eng.cfg) == codes, name
        fs = engine.flow_spec(0, 1, 0.25, 0.5, "auto", None, cfg=eng.cfg)
        assert (fs.bc_y, fs.bc_x) == codes and fs.nbins == 0 and (fs.cu, fs.cv) == (0, 1) and (fs.dx, fs.dy) == (0.25, 0.5)
        assert engine.flow_spec(2, 0, 1.0, 1.0, "wall", (16, -1.0, 1.0), cfg=eng.cfg).nbins == 16
        with pytest.raises(LnsError, match="flow boundary"):
            eng.rollout_eval_flow(x, x, boundary="torus")                # refused before anything touches a tensor
    for bad in ((0, -1.0, 1.0), (257, -1.0, 1.0), (8, -1.0), 8):
        with pytest.raises(LnsError, match="vort_hist"):
            engine.flow_spec(vort_hist=bad)

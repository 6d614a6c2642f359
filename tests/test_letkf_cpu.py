"""CPU: the localised ensemble transform Kalman filter (lns_rollout_latent_ensemble_analysis_local, its size query,
lns_op_ensemble_patch_gram, lns_op_letkf_combine, lns_op_ensemble_transform_local; include/lns.h) is declared, exported and bound
and refuses bad arguments before any device work in the documented order; the host taper (enkf.gaspari_cohn,
enkf.localization_weights) has the taper's properties; the numpy statements (tests/letkf_reference.py) agree with each other, fall
back to the global filter at a huge radius, leave far domains alone and notice the mistakes an implementation can make."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from helpers import ROOT

import etkf_reference as er  # noqa: E402
import letkf_reference as lr  # noqa: E402

LETKF_SYMBOLS = ("lns_rollout_ensemble_analysis_local_workspace_bytes", "lns_rollout_latent_ensemble_analysis_local",
                 "lns_op_ensemble_patch_gram", "lns_op_letkf_combine", "lns_op_ensemble_transform_local")
_P = ctypes.c_void_p(0x1000)                          # stands for a device pointer; never dereferenced
_T = 5


def _ints(*v):
    return (ctypes.c_int * len(v))(*v)


def _norm(size=None, per_channel=0):
    from lns_amd import _lib
    s = _lib.LnsEvalSpec()
    s.size = ctypes.sizeof(_lib.LnsEvalSpec) if size is None else size
    s.per_channel = per_channel
    s.mean, s.std, s.eps = 0.0, 1.0, 1e-8
    return s


def test_letkf_symbols_are_declared_exported_and_bound():
    from lns_amd import _lib, dropin, engine, enkf
    _lib.build()
    src = open(os.path.join(ROOT, "include", "lns.h")).read()
    for text in ("ty = (y * h) / Ly, tx = (x * w) / Lx", "dist = sqrt((double)(dy*dy + dx*dx)), r = dist / radius",
                 "rho = (((1 - (5/3) r2) + (5/8) r3) + (1/2) r4) - (1/4) r5", "S_l = sum_steps (ascending) sum_t (ascending, rho_lt > 0) rho_lt * G_t",
                 "out[b][m][ch][l] = (float)(zbar + sum_k Z_k X_l[k][m])", "loc_radius must be finite and > 0",
                 "Not there: localisation, M > 64, additive inflation"):
        assert text in src, text
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(lns_[a-z0-9_]+)\s*\(", src))
    L = ctypes.CDLL(_lib.LIB_PATH)
    for s in LETKF_SYMBOLS:
        assert s in declared, "not declared in include/lns.h: " + s
        assert hasattr(L, s), "missing export: " + s
        assert s in _lib.SYMBOLS
        assert getattr(_lib.lib(), s).argtypes, "not bound in _lib.lib(): " + s
    assert re.search(r"#define\s+LNS_ABI_VERSION\s+2\b", src)         # additive: the ABI version stays
    assert re.search(r"#define\s+LNS_LETKF_MAX_DOMAINS\s+4096\b", src)
    assert _lib.lib().lns_build_has(b"ensemble_letkf") == 1
    assert engine.LocalEnsembleAnalysis._fields == ("z", "param", "X_local", "wbar_local", "lam_local", "status_local", "X", "wbar", "lam",
                                                    "stat", "status", "mean", "var", "z_last")
    assert enkf.LocalEnKFResult._fields == ("z", "param", "X", "lam", "stat", "status", "dfs")
    assert issubclass(enkf.LocalEnsembleFilter, enkf.EnsembleFilter)
    for owner, name in ((engine.Engine, "ensemble_patch_gram"), (engine.Engine, "letkf_combine"), (engine.Engine, "ensemble_transform_local"),
                        (engine.Engine, "rollout_latent_ensemble_analysis_local"), (enkf.LocalEnsembleFilter, "analysis"),
                        (enkf.LocalEnsembleFilter, "run"), (enkf, "gaspari_cohn"), (enkf, "localization_weights")):
        assert callable(getattr(owner, name))
    import inspect
    sig = inspect.signature(dropin.LatentDynamics.assimilate_ensemble)
    assert sig.parameters["loc_radius"].default is None and sig.parameters["loc_boundary"].default == "auto"


def test_letkf_kernels_use_no_scratch():
    """tools/kernel_resources.py on the code object: the three new kernels keep their tiles in registers; one kernel per name"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    from lns_amd import _lib
    res = kernel_resources.resources(_lib.LIB_PATH)
    for name in ("letkf_patch_gram_kernelILi2", "letkf_patch_gram_kernelILi4", "letkf_combine_kernel", "letkf_update_kernel"):
        k = [v for n, v in res.items() if name in n]
        assert len(k) == 1, name
        assert k[0]["scratch"] == 0 and k[0]["vgpr_spill"] == 0, (name, k[0])


# ---- the refusal matrix ----------------------------------------------------------------------------------------------------
def _engines():
    from lns_amd import _lib, config, engine
    mini = config.preset("ns2d_mini")
    return {"full": engine.Engine(engine.make_config(mini, ae_prefix="vq_ae.", prop_prefix="propagator.")),
            "cond": engine.Engine(engine.make_config(config.preset("twophase_cond"), ae_prefix="ae.", prop_prefix="propagator.")),
            "noprop": engine.Engine(engine.make_config(mini, prop_kind=_lib.LNS_PROP_NONE, ae_prefix="vq_ae."))}


_PASSED = (-3, "lns_finalize_weights must be called first")        # every refusal passed: no weights on this machine
_BATCH = (-1, "batch 65536 exceeds the maximum of 65535 trajectories per call")
_NO_MODEL = (-3, "rollout needs autoencoder and propagator")
_KEEP_2_3 = (-1, "keep_steps must be ascending steps in [0, 5): entry 2 is 3")
_N_KEEP_1 = (-1, "n_keep must be at least 1 (for no decoded step: lns_rollout with to_x = 0)")
_B, _M, _T0 = (-1, "B must be positive"), (-1, "M must be positive"), (-1, "T must be positive")
_Y, _R, _ZA = (-1, "y_obs is null"), (-1, "rinv is null"), (-1, "z_analysis is null")
_STRIDE = (-1, "the strides of rinv must be >= 0 (0: shared)")
_RHO = (-1, "rho (the multiplicative inflation) must be finite and >= 1")
_RAD = (-1, "loc_radius must be finite and > 0")
_BC = (-1, "bc_y / bc_x must be LNS_FLOW_PERIODIC or LNS_FLOW_WALL")
_MR = (-1, "ensemble analysis needs M in 2 .. 64 (the transform keeps A and Q in LDS; 65 .. 128 members are not supported)")
_VM = (-1, "var_out needs mean_out")
_PA = (-1, "param_analysis needs param")
_NORM = (-1, "norm: the size field is not sizeof(lns_eval_spec)")
# (arguments of the call that differ from a valid one, expected (return code, message))
_REFUSALS = [
    (dict(), _PASSED), (dict(mean=None, var=None), _PASSED), (dict(last=_P), _PASSED), (dict(param=_P, pa=_P), _PASSED),
    (dict(M=2), _PASSED), (dict(M=64), _PASSED), (dict(norm=None), _PASSED), (dict(rad=1e-3), _PASSED), (dict(rad=1e9), _PASSED),
    (dict(by=1, bx=1), _PASSED), (dict(by=0, bx=0), _PASSED),
    (dict(Xl=None, wl=None, ll=None, sl=None, X=None, wbar=None, lam=None, stat=None, status=None), _PASSED),
    (dict(z=None), (-1, "z_in is null")), (dict(y=None), _Y), (dict(rinv=None), _R), (dict(za=None), _ZA),
    (dict(rbs=-1), _STRIDE), (dict(rho=0.999), _RHO), (dict(rho=float("nan")), _RHO),
    (dict(rad=0.0), _RAD), (dict(rad=-1.0), _RAD), (dict(rad=float("inf")), _RAD), (dict(rad=float("nan")), _RAD),
    (dict(by=2), _BC), (dict(bx=-1), _BC), (dict(by=7, bx=7), _BC),
    (dict(B=0), _B), (dict(M=0), _M), (dict(T=0), _T0),
    (dict(M=1), (-1, "var_out needs M >= 2")), (dict(M=1, mean=None, var=None), _MR), (dict(M=65), _MR),
    (dict(mean=None), _VM), (dict(pa=_P), _PA), (dict(norm="short"), _NORM),
    (dict(k=_ints(0, 4, 3)), _KEEP_2_3), (dict(k=None), (-1, "keep_steps is null")), (dict(nk=0), _N_KEEP_1),
    (dict(B=1024, M=64), _BATCH), (dict(eng="noprop"), _NO_MODEL),
    (dict(eng="cond"), (-1, "conditional propagator needs param")), (dict(eng="cond", param=_P, pa=_P), _PASSED),
    # two failing checks: the ETKF call's order, the two new checks directly after the one on rho
    (dict(rss=-1, rho=0.5), _STRIDE), (dict(rho=0.5, rad=0.0), _RHO), (dict(rad=0.0, by=2), _RAD), (dict(by=2, B=0), _BC),
    (dict(rad=-1.0, B=0), _RAD), (dict(bx=5, M=65), _BC), (dict(za=None, rad=0.0), _ZA), (dict(rad=0.0, eng="noprop"), _RAD),
    (dict(by=3, B=1024, M=64), _BC), (dict(M=65, mean=None), _MR), (dict(B=1024, M=64, eng="noprop"), _BATCH),
]


def _call(L, h, a, norms, nbytes=1 << 30):
    sp = ctypes.byref(norms[a["norm"]]) if a["norm"] else None
    return L.lns_rollout_latent_ensemble_analysis_local(h, a["z"], a["param"], a["y"], a["rinv"], a["rbs"], a["rss"], a["B"], a["M"], a["T"],
                                                        a["k"], a["nk"], sp, a["rho"], a["rad"], a["by"], a["bx"], a["za"], a["Xl"],
                                                        a["wl"], a["ll"], a["sl"], a["pa"], a["X"], a["wbar"], a["lam"], a["stat"],
                                                        a["status"], a["mean"], a["var"], a["last"], a["ws"], nbytes, None)


def _valid():
    return dict(eng="full", z=_P, param=None, y=_P, rinv=_P, rbs=7, rss=3, B=2, M=3, T=_T, k=_ints(0, 3, 4), nk=3, norm="ok", rho=1.25,
                rad=2.0, by=0, bx=1, za=_P, Xl=_P, wl=_P, ll=_P, sl=_P, pa=None, X=_P, wbar=_P, lam=_P, stat=_P, status=_P, mean=_P, var=_P,
                last=None, ws=_P)


def test_local_analysis_refuses_bad_arguments_without_a_device():
    """Every refusal is decided before the first HIP call (fake pointers, no device here), in the order of include/lns.h; a call
    that passes them all stops at the weights that were never finalised."""
    from lns_amd import _lib
    L = _lib.lib()
    engines = _engines()
    norms = {"ok": _norm(), "short": _norm(size=8)}
    assert _call(L, None, _valid(), norms) == _lib.LNS_EINVAL
    for kw, (want_rc, want_msg) in _REFUSALS:
        a = _valid()
        a.update(kw)
        h = engines[a["eng"]]._h
        rc = _call(L, h, a, norms)
        assert (rc, L.lns_last_error(h).decode()) == (want_rc, want_msg), kw


def test_local_workspace_query_refuses_in_order_and_holds_the_patch_sums():
    """The size query refuses as the ETKF's does; its size is the ensemble layout plus a region that holds at least the patch sums
    [B][n_keep][h*w][M*M + M + 3] and the per-domain S, g, X, wbar, lam, and grows by the patch sums per further kept step."""
    from lns_amd import _lib
    L = _lib.lib()
    engines = _engines()
    n = ctypes.c_size_t(0)
    assert L.lns_rollout_ensemble_analysis_local_workspace_bytes(None, 2, 3, 1, ctypes.byref(n)) == _lib.LNS_EINVAL
    for (eng, B, M, nk), want in ((("full", 0, 3, 1), _B), (("full", 2, 0, 1), _M), (("full", 2, 1, 1), _MR), (("full", 2, 65, 1), _MR),
                                  (("full", 2, 3, 0), (-1, "n_keep must be at least 1")), (("full", 1024, 64, 1), _BATCH),
                                  (("noprop", 2, 3, 1), _NO_MODEL), (("full", 0, 65, 0), _B), (("full", 2, 3, 1), _PASSED)):
        h = engines[eng]._h
        rc = L.lns_rollout_ensemble_analysis_local_workspace_bytes(h, B, M, nk, ctypes.byref(n))
        assert (rc, L.lns_last_error(h).decode()) == want, (eng, B, M, nk)


def test_letkf_ops_refuse_bad_arguments_without_a_device():
    """The three ops: code, message (under the op's name, lns_create_error) and order."""
    from lns_amd import _lib
    L = _lib.lib()
    ok, short, pc = _norm(), _norm(size=8), _norm(per_channel=1)
    members, grid = "M in 2 .. 64", "h, w >= 1 and h * w <= 4096"

    def gram(frames=_P, y=_P, rinv=_P, rbs=0, rss=0, n=2, B=2, M=3, C=3, H=4, W=5, h=2, w=2, norm=ok, part=_P):
        return L.lns_op_ensemble_patch_gram(frames, y, rinv, rbs, rss, n, B, M, C, H, W, h, w, ctypes.byref(norm) if norm is not None else None,
                                            part, None)

    def combine(part=_P, B=2, n=2, M=3, h=2, w=3, rad=1.0, by=0, bx=1, Sl=_P, gl=_P, Sg=_P, gg=_P, stat=_P):
        return L.lns_op_letkf_combine(part, B, n, M, h, w, rad, by, bx, Sl, gl, Sg, gg, stat, None)

    def update(z=_P, X=_P, B=2, M=3, c=4, h=2, w=3, out=_P):
        return L.lns_op_ensemble_transform_local(z, X, B, M, c, h, w, out, None)
    null_in = "frames, y_obs or rinv is null"
    outs = "S_local, g_local, S_glob or g_glob is null"
    for fn, prefix, cases in (
        (gram, "ensemble_patch_gram: ", (
            (dict(frames=None), null_in), (dict(y=None), null_in), (dict(rinv=None), null_in), (dict(part=None), "part_out is null"),
            (dict(norm=short), "spec is null or its size"), (dict(M=1), members), (dict(M=65), members), (dict(n=0), "n >= 1"),
            (dict(B=0), "B in"), (dict(C=0), "C, H, W"), (dict(n=65536, B=1, C=1), "n in 1..65535"), (dict(h=0), grid), (dict(w=-1), grid),
            (dict(h=65, w=64), grid), (dict(rbs=-1), "strides of rinv"), (dict(C=9, norm=pc), "per-channel form needs C <= 8"),
            (dict(frames=None, part=None), null_in), (dict(part=None, norm=short), "part_out is null"), (dict(M=65, n=0), members),
            (dict(n=0, h=0), "n >= 1"), (dict(h=0, rss=-1), grid))),
        (combine, "letkf_combine: ", (
            (dict(part=None), "part is null"), (dict(Sl=None), outs), (dict(gl=None), outs), (dict(Sg=None), outs), (dict(gg=None), outs),
            (dict(M=1), members), (dict(M=65), members), (dict(B=0), "B in 1..65535, n >= 1"), (dict(n=0), "B in 1..65535, n >= 1"),
            (dict(h=0), grid), (dict(h=64, w=65), grid), (dict(rad=0.0), "loc_radius must be finite and > 0"),
            (dict(rad=float("nan")), "loc_radius must be finite and > 0"), (dict(rad=float("inf")), "loc_radius must be finite and > 0"),
            (dict(by=2), "bc_y / bc_x must be"), (dict(bx=-1), "bc_y / bc_x must be"),
            (dict(part=None, Sl=None), "part is null"), (dict(gg=None, M=65), outs), (dict(M=65, B=0), members), (dict(h=0, rad=0.0), grid),
            (dict(rad=0.0, by=2), "loc_radius must be finite and > 0"))),
        (update, "ensemble_transform_local: ", (
            (dict(z=None), "z, X_local or out is null"), (dict(X=None), "z, X_local or out is null"), (dict(out=None), "z, X_local or out is null"),
            (dict(M=1), members), (dict(M=65), members), (dict(B=0), "B in 1..65535"), (dict(c=0), "c in 1..65536"), (dict(h=0), grid),
            (dict(h=4097, w=1), grid), (dict(z=None, M=65), "z, X_local or out is null"), (dict(M=65, B=0), members), (dict(c=0, w=0), "c in 1..65536"))),
    ):
        for kw, word in cases:
            assert fn(**kw) == _lib.LNS_EINVAL, (prefix, kw)
            msg = L.lns_create_error().decode()
            assert msg.startswith(prefix) and word in msg, (kw, msg)


# ---- the taper on the host ---------------------------------------------------------------------------------------------------
def test_gaspari_cohn_has_the_tapers_properties():
    """1 at 0; 5/24 at r = 1 from both branches to 1e-15; exactly 0 from 2 on; never negative below 2; non-increasing, up to the
    rounding of its six terms (each at most 10.7 in magnitude just below 2: 6 x 2^-53 x 16 < 1.1e-14); the reference's float64
    taper gives the same bits."""
    from lns_amd import enkf
    gc = enkf.gaspari_cohn
    assert gc(0.0) == 1.0 and gc(np.float64(0.0)).dtype == np.float64
    assert abs(float(gc(1.0)) - 5.0 / 24.0) <= 1e-15
    just_above = float(gc(np.nextafter(1.0, 2.0)))               # the 1 < r < 2 branch next to r = 1
    assert abs(just_above - 5.0 / 24.0) <= 1e-15
    r = 1.0
    far_at_1 = (((((4.0 - 5.0 * r) + (5.0 / 3.0)) + (5.0 / 8.0)) - 0.5) + (1.0 / 12.0)) - 2.0 / 3.0       # the far polynomial at r = 1
    assert abs(far_at_1 - 5.0 / 24.0) <= 1e-15
    for far in (2.0, np.nextafter(2.0, 3.0), 2.5, 1e9, np.inf):
        assert gc(far) == 0.0
    grid = np.concatenate([np.linspace(0.0, 2.0, 200001), 2.0 - np.geomspace(1e-16, 1e-2, 400)])
    grid.sort()
    v = gc(grid)
    assert (v >= 0.0).all() and (v <= 1.0).all()
    assert (np.diff(v) <= 1.1e-14).all(), np.diff(v).max()
    assert np.array_equal(v, lr.taper(grid))
    assert np.abs(v - lr.taper(grid, lr.LD).astype(np.float64)).max() <= 1.1e-14


def test_localization_weights_wrap_on_a_periodic_axis_only():
    from lns_amd import enkf
    lw = enkf.localization_weights
    for h in (2, 5):
        per = lw(h, 3, 1.5, ("periodic", "wall")).reshape(h, 3, h, 3)
        wall = lw(h, 3, 1.5, ("wall", "wall")).reshape(h, 3, h, 3)
        gc = enkf.gaspari_cohn
        # rows 0 and h - 1 are one apart on the periodic axis, h - 1 apart against a wall
        assert per[0, 1, h - 1, 1] == gc(1.0 / 1.5)
        assert wall[0, 1, h - 1, 1] == gc((h - 1) / 1.5)
        if h == 5:
            assert per[0, 0, 3, 0] == gc(2.0 / 1.5) and wall[0, 0, 3, 0] == 0.0 and per[0, 0, 2, 0] == wall[0, 0, 2, 0]
        # x is a wall in both: columns 0 and 2 are two apart
        assert per[0, 0, 0, 2] == gc(2.0 / 1.5) == wall[0, 0, 0, 2]
        xper = lw(h, 3, 1.5, ("wall", "periodic")).reshape(h, 3, h, 3)
        assert xper[0, 0, 0, 2] == gc(1.0 / 1.5)
        for m in (per, wall, xper):
            flat = m.reshape(h * 3, h * 3)
            assert np.array_equal(flat, flat.T) and (np.diag(flat) == 1.0).all()
        for bc, name in (((0, 1), ("periodic", "wall")), ((1, 1), "wall"), ((0, 0), "periodic")):
            assert np.array_equal(lw(h, 3, 1.5, name), lr.weights(h, 3, 1.5, bc))
    assert np.array_equal(lw(4, 4, 0.5, "periodic"), np.eye(16))           # radius 0.5: the own patch only
    assert lw(4, 4, 1.0, "wall").reshape(4, 4, 4, 4)[0, 0, 2, 0] == 0.0    # dist = 2 radius: exactly 0
    from lns_amd._lib import LnsError
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(LnsError):
            lw(2, 2, bad, "wall")


# ---- the statements ----------------------------------------------------------------------------------------------------------
def _case(M, seed, grid=(2, 3), plane=(5, 7), C=2, n=2, B=1, c=3):
    fr, yy = er.family_inputs((n, B, M, C) + plane, seed, "normal")
    r = er.rinv_map((B, n, C) + plane, seed + 1, density=0.6)
    z = np.random.default_rng(seed + 2).standard_normal((B, M, c) + grid).astype(np.float32)
    return fr, yy, r, z


@pytest.mark.parametrize("M", [2, 7, 33, 64])
def test_order_exact_form_equals_the_independent_form_under_the_rule(M):
    """Patch sums -> combine -> transform per domain -> update (the device's route, float64) against the independent statement
    (per-value weights rinv_p * rho(l, patch(p)), no patch sums) in longdouble, under max(1e-12, 3 x own), own = the independent
    float64 form against its longdouble form: S_l, g_l, X_l, lam_l and the analysis latents; a 5 x 7 plane on 2 x 3 patches of
    unequal size (2 x 2 at M = 64: the longdouble Jacobi takes a second per domain), periodic in y and a wall in x, radius 1.2."""
    grid = (2, 2) if M == 64 else (2, 3)
    fr, yy, r, z = _case(M, 500 + M, grid=grid)
    bc = (lr.PERIODIC, lr.WALL)
    for norm in (None, dict(mean=0.3, std=1.7)):
        got = lr.exact_analysis(fr, yy, r, z, 1.3, grid, 1.2, bc, norm)
        i64 = lr.local_analysis(fr, yy, r, z, 1.3, grid, 1.2, bc, norm)
        ild = lr.local_analysis(fr, yy, r, z, 1.3, grid, 1.2, bc, norm, dt=lr.LD)
        assert (got["status"] == 0).all() and (i64["status"] == 0).all()
        for k in ("S", "g", "X", "lam", "z"):
            ok, ratio, dist, lim = er.held(got[k], i64[k], ild[k])
            print("M=%d %s: %.3g of the bound" % (M, k, ratio))
            assert ok, (M, k, dist, lim)


@pytest.mark.parametrize("M", [2, 7, 33])
def test_local_domains_equal_the_state_space_kalman_formulas(M):
    """The observed plane itself as the state: under the weights rinv_p * rho(l, patch(p)) of domain l the mean of the members
    transformed by X_l equals xbar + K (y - H xbar), K = P H^T (H P H^T + R_l)^-1 (etkf_reference.kalman, float64, written
    independently), under the rule, own = the float64 mean against the longdouble mean."""
    grid, plane = (2, 2), (4, 6)
    fr, yy = er.family_inputs((1, 1, M, 1) + plane, 900 + M, "normal")
    r = er.rinv_map((1, 1, 1) + plane, 901 + M, density=0.7, per_sample=False, per_step=False)
    bc = (lr.WALL, lr.WALL)
    z = np.zeros((1, M, 1) + grid, dtype=np.float32)
    a64 = lr.local_analysis(fr, yy, r, z, 1.3, grid, 1.0, bc)
    ald = lr.local_analysis(fr, yy, r, z, 1.3, grid, 1.0, bc, dt=lr.LD)
    rho = lr.weights(2, 2, 1.0, bc)
    pidx = lr.patch_index(4, 6, 2, 2)
    members = fr[0, 0].reshape(M, -1)
    for l in range(4):
        rl = r.reshape(-1).astype(np.float64) * rho[l][pidx].reshape(-1)
        want_mean, _ = er.kalman(members, yy[0, 0].reshape(-1), rl, 1.3)
        state = members[None]                                          # [1, M, N]: the plane as the state
        m64 = er.update(state, a64["X"][:, l], rounded=False)[0].mean(0)
        mld = er.update(state, ald["X"][:, l], dt=lr.LD, rounded=False)[0]
        mld = mld.sum(0) / lr.LD(M)
        lim = er.bound(er.distance(m64, mld))
        dist = er.distance(m64, want_mean)
        assert dist[0] <= lim[0] and dist[1] <= lim[1], (M, l, dist, lim)


@pytest.mark.parametrize("M", [2, 7, 33, 64])
def test_a_huge_radius_gives_the_global_transform(M):
    """radius = 1e9: every rho is 1 to the last bit (1 - 5/3 r^2 rounds to 1), so every X_l equals the global
    etkf_reference.transform of the summed Gram under the rule, and so does the global transform of the device's route."""
    grid = (2, 2) if M == 64 else (2, 3)
    fr, yy, r, z = _case(M, 700 + M, grid=grid)
    assert np.array_equal(lr.weights(grid[0], grid[1], 1e9, (1, 1)), np.ones((grid[0] * grid[1],) * 2))
    got = lr.exact_analysis(fr, yy, r, z, 1.3, grid, 1e9, (lr.WALL, lr.PERIODIC))
    S64, g64, _ = er.gram(fr, yy, r)
    Sld, gld, _ = er.gram(fr, yy, r, dt=er.LD)
    X64, Xld = er.transform(S64, g64, 1.3)[0], er.transform(Sld, gld, 1.3, dt=er.LD)[0]
    for l in range(grid[0] * grid[1]):
        ok, ratio, dist, lim = er.held(got["X"][:, l], X64, Xld)
        assert ok, (M, l, dist, lim)
    ok, ratio, dist, lim = er.held(got["Xg"], X64, Xld)
    assert ok, (M, "global", dist, lim)
    assert np.array_equal(got["stat"][:, :, 2], (np.broadcast_to(r, yy.shape) > 0).sum((2, 3, 4)))


def test_far_domains_keep_their_forecast_members():
    """Observations confined to one patch: every domain at dist >= 2 radius has S_l = 0 and X_l = sqrt(rho) I exactly (rho = 4:
    (M - 1) / rho and sqrt(rho) are exact), wbar = 0, in both statements; the domains inside the support move."""
    M, grid, plane = 5, (4, 5), (9, 11)
    fr, yy = er.family_inputs((1, 2, M, 2) + plane, 77, "normal")
    pidx = lr.patch_index(9, 11, 4, 5)
    own = 1 * 5 + 2                                                      # patch (1, 2)
    r = np.where(pidx == own, np.float32(1.5), np.float32(0.0))[None].repeat(2, 0)      # [C, H, W]
    z = np.random.default_rng(3).standard_normal((2, M, 3) + grid).astype(np.float32)
    bc = (lr.WALL, lr.WALL)
    for radius in (0.5, 1.0):
        for a in (lr.exact_analysis(fr, yy, r, z, 4.0, grid, radius, bc), lr.local_analysis(fr, yy, r, z, 4.0, grid, radius, bc)):
            for l in range(20):
                dist = np.hypot(l // 5 - 1, l % 5 - 2)
                if dist >= 2 * radius:
                    assert not a["S"][:, l].any() and not a["wbar"][:, l].any(), (radius, l)
                    assert np.array_equal(a["X"][:, l], np.broadcast_to(2.0 * np.eye(M), (2, M, M))), (radius, l)
                else:
                    assert a["S"][:, l].any() and not np.array_equal(a["X"][0, l], 2.0 * np.eye(M)), (radius, l)


def test_reference_notices_four_deliberate_mistakes():
    """ty / tx swapped, wrap on a wall axis, the taper applied twice, the domain's X taken from its neighbour: each moves X_l or the
    analysis latents by at least 100 x the rule's bound on these inputs; the unmutated copy does not."""
    M, grid = 7, (3, 4)
    fr, yy = er.family_inputs((1, 1, M, 2, 9, 8), 31, "normal")
    r = (er.rinv_map((1, 1, 2, 9, 8), 32, density=0.4) * np.float32(3.0)).astype(np.float32)
    z = np.random.default_rng(33).standard_normal((1, M, 2) + grid).astype(np.float32)
    bc = (lr.WALL, lr.PERIODIC)
    a64 = lr.local_analysis(fr, yy, r, z, 1.3, grid, 1.0, bc)
    ald = lr.local_analysis(fr, yy, r, z, 1.3, grid, 1.0, bc, dt=lr.LD)
    lims = {k: er.bound(er.distance(a64[k], ald[k])) for k in ("X", "z")}
    for kind in (None, "tytx_swapped", "wrap_on_wall", "taper_twice", "neighbour_X"):
        got = lr.local_analysis(fr, yy, r, z, 1.3, grid, 1.0, bc, mistake=kind)
        moved = max(max(d / b for d, b in zip(er.distance(got[k], ald[k]), lims[k])) for k in ("X", "z"))
        print("%s: %.3g x the bound" % (kind, moved))
        assert (moved <= 1.0) if kind is None else (moved >= 100.0), (kind, moved)

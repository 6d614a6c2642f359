"""CPU: the ensemble exceedance tables (lns_rollout_latent_ensemble_exceed, lns_op_ensemble_exceed, include/lns.h) are
declared, exported and bound and refuse bad arguments before any device work in the documented order; the stored-path
statement `metrics.exceedance_table` equals the independent reference (tests/ensemble_exceed_reference.py) count for count;
the scores of `lns_amd.metrics` equal their per-pixel definitions; and the reference notices the mistakes an implementation
can make."""
import copy
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from helpers import ROOT

import ensemble_exceed_reference as ref  # noqa: E402

EXCEED_SYMBOLS = ("lns_rollout_latent_ensemble_exceed", "lns_op_ensemble_exceed")
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


def _xspec(n_thr=2, size=None):
    from lns_amd import _lib
    s = _lib.LnsEnsembleExceedSpec()
    s.size = ctypes.sizeof(_lib.LnsEnsembleExceedSpec) if size is None else size
    s.n_thr = n_thr
    return s


def test_exceed_symbols_are_declared_exported_and_bound():
    from lns_amd import _lib, dropin, engine, metrics
    _lib.build()
    src = open(os.path.join(ROOT, "include", "lns.h")).read()
    for text in ("n = #{m : v_m > thr[k][c]}", "o = (q > thr[k][c]) ? 1 : 0", "a NaN compares false in both comparisons",
                 "table[b][i][k][c][o][n]", "[B][n_keep][n_thr][Cin][2][M+1]", "The call overwrites the whole table"):
        assert text in src, text
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(lns_[a-z0-9_]+)\s*\(", src))
    L = ctypes.CDLL(_lib.LIB_PATH)
    for s in EXCEED_SYMBOLS:
        assert s in declared, "not declared in include/lns.h: " + s
        assert hasattr(L, s), "missing export: " + s
        assert s in _lib.SYMBOLS
        assert getattr(_lib.lib(), s).argtypes, "not bound in _lib.lib(): " + s
    assert re.search(r"#define\s+LNS_ABI_VERSION\s+2\b", src)         # additive: the ABI version stays
    assert "lns_ensemble_exceed_spec" in src
    assert ctypes.sizeof(_lib.LnsEnsembleExceedSpec) == 8 + 8 * 8 * 4
    assert _lib.lib().lns_build_has(b"ensemble_exceed") == 1
    assert _lib.lib().lns_build_has(b"ensemble_quantiles") == 1
    assert engine.EnsembleExceedance._fields == ("table", "mean", "var", "z_last")
    for owner, name in ((engine.Engine, "ensemble_exceed"), (engine.Engine, "rollout_latent_ensemble_exceed"),
                        (dropin.LatentDynamics, "validate_exceedance"), (metrics, "exceedance_table"), (metrics, "brier_scores"),
                        (metrics, "reliability_curve"), (metrics, "roc_curve"), (metrics, "contingency_scores")):
        assert callable(getattr(owner, name))


def test_exceed_kernel_uses_no_scratch_and_spills_nothing():
    """tools/kernel_resources.py on the code object: the eight counters stay in registers"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    from lns_amd import _lib
    res = kernel_resources.resources(_lib.LIB_PATH)
    k = [v for n, v in res.items() if "ensemble_exceed_kernel" in n]
    assert len(k) == 1
    assert k[0]["scratch"] == 0 and k[0]["vgpr_spill"] == 0 and k[0]["sgpr_spill"] == 0, k[0]


def _engines():
    from lns_amd import _lib, config, engine
    mini = config.preset("ns2d_mini")
    wide = copy.copy(mini)
    wide.in_channels = 9
    return {"full": engine.Engine(engine.make_config(mini, ae_prefix="vq_ae.", prop_prefix="propagator.")),
            "cond": engine.Engine(engine.make_config(config.preset("twophase_cond"), ae_prefix="ae.", prop_prefix="propagator.")),
            "noprop": engine.Engine(engine.make_config(mini, prop_kind=_lib.LNS_PROP_NONE, ae_prefix="vq_ae.")),
            "wide": engine.Engine(engine.make_config(wide, ae_prefix="vq_ae.", prop_prefix="propagator."))}


_PASSED = (-3, "lns_finalize_weights must be called first")        # every refusal passed: no weights on this machine
_BATCH = (-1, "batch 65536 exceeds the maximum of 65535 trajectories per call")
_NO_MODEL = (-3, "rollout needs autoencoder and propagator")
_KEEP_2_3 = (-1, "keep_steps must be ascending steps in [0, 5): entry 2 is 3")
_N_KEEP_1 = (-1, "n_keep must be at least 1 (for no decoded step: lns_rollout with to_x = 0)")
_B, _M, _T0 = (-1, "B must be positive"), (-1, "M must be positive"), (-1, "T must be positive")
_Y = (-1, "y_true is null")
_XS = (-1, "xspec is null or its size field is not sizeof(lns_ensemble_exceed_spec)")
_NT = (-1, "xspec: n_thr must be in 1 .. 8")
_TO = (-1, "table_out is null")
_MR = (-1, "ensemble exceedance needs M in 1 .. 128")
_VM, _V2 = (-1, "var_out needs mean_out"), (-1, "var_out needs M >= 2")
_NORM = (-1, "norm: the size field is not sizeof(lns_eval_spec)")
_CH = (-1, "thresholds need in_channels <= 8")
# (arguments of the call that differ from a valid one, expected (return code, message))
_REFUSALS = [
    (dict(), _PASSED), (dict(mean=None, var=None), _PASSED), (dict(var=None), _PASSED), (dict(last=_P), _PASSED),
    (dict(param=_P), _PASSED), (dict(ws=None), _PASSED), (dict(M=1, var=None), _PASSED), (dict(M=128), _PASSED),
    (dict(B=511, M=128), _PASSED), (dict(norm=None), _PASSED), (dict(norm="per_channel"), _PASSED),
    (dict(xs="one"), _PASSED), (dict(xs="eight"), _PASSED),
    (dict(z=None), (-1, "z_in is null")),
    (dict(y=None), _Y),
    (dict(xs=None), _XS), (dict(xs="short"), _XS),
    (dict(xs="zero"), _NT), (dict(xs="neg"), _NT), (dict(xs="nine"), _NT),
    (dict(table=None), _TO),
    (dict(B=0), _B), (dict(B=-1), _B), (dict(M=0), _M), (dict(M=-1), _M), (dict(T=0), _T0), (dict(T=-1), _T0),
    (dict(M=1), _V2), (dict(M=129), _MR), (dict(M=129, mean=None, var=None), _MR),
    (dict(mean=None), _VM),
    (dict(norm="short"), _NORM),
    (dict(eng="wide"), _CH), (dict(eng="wide", norm=None), _CH),
    (dict(eng="wide", norm="per_channel"), _CH),                   # (this form has no per-channel norm check of its own)
    (dict(k=_ints(0, 4, 3)), _KEEP_2_3), (dict(k=None), (-1, "keep_steps is null")),
    (dict(nk=0), _N_KEEP_1), (dict(nk=-1), _N_KEEP_1),
    (dict(B=512, M=128), _BATCH),
    (dict(eng="noprop"), _NO_MODEL),
    (dict(eng="cond"), (-1, "conditional propagator needs param")), (dict(eng="cond", param=_P), _PASSED),
    # two failing checks: arguments (in the order of the list above), then the batch, then the model, then param
    (dict(z=None, y=None), (-1, "z_in is null")), (dict(y=None, xs=None), _Y), (dict(xs=None, table=None), _XS),
    (dict(xs="nine", table=None), _NT), (dict(table=None, B=0), _TO), (dict(xs="zero", B=0), _NT),
    (dict(B=0, M=0), _B), (dict(M=0, T=0), _M), (dict(T=0, M=129), _T0), (dict(M=129, mean=None), _MR),
    (dict(mean=None, norm="short"), _VM), (dict(norm="short", eng="wide"), _NORM), (dict(eng="wide", nk=0), _CH),
    (dict(norm="short", nk=0), _NORM), (dict(nk=0, k=None), _N_KEEP_1),
    (dict(k=_ints(0, 4, 3), B=512, M=128), _KEEP_2_3), (dict(norm="short", B=512, M=128), _NORM),
    (dict(xs=None, eng="noprop"), _XS), (dict(B=512, M=128, eng="noprop"), _BATCH),
    (dict(B=512, M=128, eng="cond"), _BATCH), (dict(M=129, eng="cond"), _MR), (dict(eng="noprop", param=_P), _NO_MODEL),
]


def _xspecs():
    return {"ok": _xspec(), "short": _xspec(size=8), "one": _xspec(1), "eight": _xspec(8), "zero": _xspec(0), "neg": _xspec(-1),
            "nine": _xspec(9)}


def test_ensemble_exceed_refuses_bad_arguments_without_a_device():
    """Every refusal is decided before the first HIP call (fake pointers, no device here), in the order arguments, batch
    (on B * M), model, param; a call that passes them all stops at the weights that were never finalised."""
    from lns_amd import _lib
    L = _lib.lib()
    engines = _engines()
    norms = {"ok": _norm(), "short": _norm(size=8), "per_channel": _norm(per_channel=1)}
    xspecs = _xspecs()
    assert L.lns_rollout_latent_ensemble_exceed(None, _P, None, _P, 2, 3, _T, _ints(0, 3, 4), 3, ctypes.byref(xspecs["ok"]), None, _P,
                                                _P, _P, None, _P, 1 << 30, None) == _lib.LNS_EINVAL
    for kw, (want_rc, want_msg) in _REFUSALS:
        a = dict(eng="full", z=_P, param=None, y=_P, B=2, M=3, T=_T, k=_ints(0, 3, 4), nk=3, xs="ok", norm="ok", table=_P,
                 mean=_P, var=_P, last=None, ws=_P)
        a.update(kw)
        h = engines[a["eng"]]._h
        xp = ctypes.byref(xspecs[a["xs"]]) if a["xs"] else None
        sp = ctypes.byref(norms[a["norm"]]) if a["norm"] else None
        rc = L.lns_rollout_latent_ensemble_exceed(h, a["z"], a["param"], a["y"], a["B"], a["M"], a["T"], a["k"], a["nk"], xp, sp,
                                                  a["table"], a["mean"], a["var"], a["last"], a["ws"], 1 << 30, None)
        assert (rc, L.lns_last_error(h).decode()) == (want_rc, want_msg), kw


def test_ensemble_exceed_op_refuses_bad_arguments_without_a_device():
    from lns_amd import _lib
    L = _lib.lib()
    ok, short = _norm(), _norm(size=8)
    xs = _xspecs()

    def op(frames=_P, y=_P, n=2, B=2, M=3, C=3, H=4, W=5, x="ok", norm=ok, table=_P):
        return L.lns_op_ensemble_exceed(frames, y, n, B, M, C, H, W, ctypes.byref(xs[x]) if x else None,
                                        ctypes.byref(norm) if norm is not None else None, table, None)
    for kw, word in ((dict(frames=None), "frames or y is null"), (dict(y=None), "frames or y is null"), (dict(x=None), "xspec is null"),
                     (dict(x="short"), "xspec is null"), (dict(x="zero"), "1 .. 8"), (dict(x="nine"), "1 .. 8"),
                     (dict(table=None), "table_out is null"), (dict(norm=short), "spec is null or its size"),
                     (dict(M=0), "M in 1 .. 128"), (dict(M=129), "M in 1 .. 128"),
                     (dict(n=0), "n >= 1"), (dict(B=0), "B in"), (dict(B=65536), "B in"), (dict(C=0), "C, H, W"), (dict(H=0), "C, H, W"),
                     (dict(W=-1), "C, H, W"), (dict(H=1 << 16, W=1 << 15), "H * W"), (dict(n=1 << 16, B=1 << 15, C=8), "n * B * C"),
                     (dict(C=9), "thresholds need C <= 8"), (dict(C=9, norm=None), "thresholds need C <= 8"),
                     # two failing checks: the order of the list above
                     (dict(frames=None, x=None), "frames or y is null"), (dict(x="nine", table=None), "1 .. 8"),
                     (dict(table=None, norm=short), "table_out is null"), (dict(norm=short, M=0), "spec is null or its size"),
                     (dict(M=129, n=0), "M in 1 .. 128"), (dict(n=0, C=9), "n >= 1")):
        assert op(**kw) == _lib.LNS_EINVAL, kw
        msg = L.lns_create_error().decode()
        assert msg.startswith("ensemble_exceed: ") and word in msg, (kw, msg)


# ---- the statement and the scores (CPU) -------------------------------------------------------------------------------------
torch = pytest.importorskip("torch")

SCALAR, per_channel_norm, thresholds_for, family_fields = ref.SCALAR, ref.per_channel_norm, ref.thresholds_for, ref.family_fields


def _metrics_table(frames, y, thr, norm):
    from lns_amd import metrics
    fields = torch.from_numpy(frames).permute(1, 2, 0, 3, 4, 5).contiguous()          # [B, M, n, C, H, W]
    return metrics.exceedance_table(fields, torch.from_numpy(y), thr, **(norm or {})).numpy()


@pytest.mark.parametrize("m", [1, 2, 3, 33])
def test_metrics_table_equals_the_reference_count_for_count(m):
    """B in {1, 3} x n in {1, 2} x C in {1, 3} x planes 1x1, 1x7, 3x5, 17x16, without a norm, with the scalar one and with the
    per-channel one (walls, clamp); eight thresholds and one; planes below 64 pixels under every shift of the family cycle.
    Every [b][i][k][c] slice sums to H * W."""
    seen = np.zeros(3, dtype=bool)
    for b in (1, 3):
        for n in (1, 2):
            for c in (1, 3):
                for (h, w) in ((1, 1), (1, 7), (3, 5), (17, 16)):
                    for shift in (range(5) if b * n * c * h * w < 64 else (0,)):
                        frames, y = family_fields((n, b, m, c, h, w), 100 * m + 7 * h + w + shift, shift)
                        seen |= np.array([np.isnan(frames).any(), np.isinf(frames).any(), np.isnan(y).any()])
                        for norm in (None, SCALAR, per_channel_norm(c)):
                            thr = thresholds_for(c)
                            want = ref.table(frames, y, thr, norm)
                            got = _metrics_table(frames, y, thr, norm)
                            assert got.dtype == np.int32 and got.shape == (b, n, 8, c, 2, m + 1)
                            assert np.array_equal(got, want), (m, b, n, c, h, w, shift, norm)
                            assert (got.sum((-1, -2)) == h * w).all()
                            assert np.array_equal(_metrics_table(frames, y, thr[:1], norm), want[:, :, :1])
    assert seen.all()


def _pixels(m, seed, h=6, w=9):
    """one plane, one threshold: (table [2, M + 1], n [pixels], o [pixels], x [M, pixels]) of gaussian members around a smooth
    truth, so every forecast value and both outcomes occur"""
    rng = np.random.default_rng(seed)
    truth = rng.standard_normal((1, 1, 1, h, w)).astype(np.float32)
    frames = (truth[None] * 0.7 + 0.6 * rng.standard_normal((1, 1, m, 1, h, w))).astype(np.float32)
    thr = (0.1,)
    x, o = ref.events(frames, truth, thr)
    nn, oo = ref.counts(frames, truth, thr)
    return ref.table(frames, truth, thr)[0, 0, 0, 0], nn.reshape(-1), oo.reshape(-1), x[0, 0, 0, :, 0].reshape(m, -1)


@pytest.mark.parametrize("m", [1, 2, 3, 33])
def test_scores_equal_their_per_pixel_definitions(m):
    """brier_scores against mean((n / M - o)^2), the per-pixel fair form and the looped decomposition, to 1e-12; bs = rel - res
    + unc; AUC against the Mann-Whitney statistic counted over all pixel pairs of a 54-pixel plane; the reliability curve and
    the ROC end points; the sequence-wise form from the summed table."""
    from lns_amd import metrics
    t, n, o, x = _pixels(m, 40 + m)
    assert 0 < o.sum() < o.size
    s = metrics.brier_scores(t)
    assert abs(float(s.bs) - ref.brier(n, o, m)) <= 1e-12
    assert abs(float(s.bs_fair) - ref.brier_fair(x, o)) <= 1e-12
    rel, res, unc, base = ref.brier_terms(n, o, m)
    assert max(abs(float(s.reliability) - rel), abs(float(s.resolution) - res), abs(float(s.uncertainty) - unc),
               abs(float(s.base_rate) - base)) <= 1e-12
    assert abs(float(s.bs) - (float(s.reliability) - float(s.resolution) + float(s.uncertainty))) <= 1e-12
    if m == 1:
        assert float(s.bs_fair) == float(s.bs)
    roc = metrics.roc_curve(t)
    assert roc.pofd.shape == (m + 2,) and roc.pod.shape == (m + 2,)
    assert (roc.pofd[0], roc.pod[0], roc.pofd[-1], roc.pod[-1]) == (0.0, 0.0, 1.0, 1.0)
    assert (np.diff(roc.pofd) >= 0).all() and (np.diff(roc.pod) >= 0).all()
    assert abs(float(roc.auc) - ref.mann_whitney(n, o)) <= 1e-12
    p, obar, cnt = metrics.reliability_curve(t)
    assert np.array_equal(p, np.arange(m + 1) / m) and np.array_equal(cnt, np.bincount(n, minlength=m + 1))
    for j in range(m + 1):
        assert (np.isnan(obar[j]) and cnt[j] == 0) or abs(obar[j] - o[n == j].mean()) <= 1e-15
    # a stack of tables is scored slice by slice, and the sequence-wise score is the score of the summed table
    t2, n2, o2, _ = _pixels(m, 90 + m)
    both = np.stack([t, t2])[None]                                            # [B = 1, n = 2, 2, M + 1]
    fs = metrics.brier_scores(torch.from_numpy(both))
    assert fs.bs.shape == (1, 2) and abs(float(fs.bs[0, 1]) - ref.brier(n2, o2, m)) <= 1e-12
    seq = metrics.brier_scores(torch.from_numpy(both).sum(1, dtype=torch.int64))
    assert abs(float(seq.bs[0]) - ref.brier(np.concatenate([n, n2]), np.concatenate([o, o2]), m)) <= 1e-12


def test_csi_of_one_member_is_the_iou_of_the_two_masks():
    from lns_amd import metrics
    t, n, o, x = _pixels(1, 7)
    s = metrics.contingency_scores(t, 1)
    f, tr = x[0].astype(bool), o.astype(bool)
    assert (int(s.hits), int(s.misses), int(s.false_alarms), int(s.correct_negatives)) == \
        (int((f & tr).sum()), int((~f & tr).sum()), int((f & ~tr).sum()), int((~f & ~tr).sum()))
    assert abs(float(s.csi) - ref.iou(f, tr)) <= 1e-15
    assert abs(float(s.pod) - (f & tr).sum() / tr.sum()) <= 1e-15 and abs(float(s.far) - (f & ~tr).sum() / f.sum()) <= 1e-15
    # M = 5, "at least 3 members": the majority mask
    t5, n5, o5, _ = _pixels(5, 8)
    assert abs(float(metrics.contingency_scores(t5, 3).csi) - ref.iou(n5 >= 3, o5.astype(bool))) <= 1e-15
    for bad in (0, 6):
        with pytest.raises(ValueError):
            metrics.contingency_scores(t5, bad)


def test_degenerate_tables_give_the_documented_values():
    """event never, event always, all members agreeing, an empty table: finite where documented, NaN where documented, never an
    exception or an infinity"""
    from lns_amd import metrics
    M = 4
    never = np.zeros((2, M + 1), dtype=np.int32)
    never[0] = (10, 5, 3, 1, 1)
    always = never[::-1].copy()
    agree = np.zeros((2, M + 1), dtype=np.int32)
    agree[0, 0], agree[0, M], agree[1, 0], agree[1, M] = 7, 2, 3, 8
    empty = np.zeros((2, M + 1), dtype=np.int32)
    with np.errstate(all="raise"):
        s = metrics.brier_scores(never)
        assert (float(s.base_rate), float(s.uncertainty), float(s.resolution)) == (0.0, 0.0, 0.0)
        assert float(s.bs) == float(s.reliability) == (5 * 0.0625 + 3 * 0.25 + 0.5625 + 1.0) / 20
        r = metrics.roc_curve(never)
        assert np.isnan(r.auc) and np.isnan(r.pod).all() and r.pofd[-1] == 1.0 and not np.isinf(r.pofd).any()
        c = metrics.contingency_scores(never, 2)
        assert (int(c.hits), int(c.misses), int(c.false_alarms), int(c.correct_negatives)) == (0, 0, 5, 15)
        assert np.isnan(c.pod) and float(c.far) == 1.0 and float(c.csi) == 0.0
        s = metrics.brier_scores(always)
        assert (float(s.base_rate), float(s.uncertainty), float(s.resolution)) == (1.0, 0.0, 0.0) and float(s.bs) == float(s.reliability)
        r = metrics.roc_curve(always)
        assert np.isnan(r.auc) and np.isnan(r.pofd).all() and r.pod[-1] == 1.0
        c = metrics.contingency_scores(always, M)
        assert (int(c.hits), int(c.misses), int(c.false_alarms), int(c.correct_negatives)) == (1, 19, 0, 0)
        assert (float(c.pod), float(c.far), float(c.csi)) == (0.05, 0.0, 0.05)
        s = metrics.brier_scores(agree)
        assert float(s.bs_fair) == float(s.bs) == (2 + 3) / 20
        assert abs(float(s.bs) - (float(s.reliability) - float(s.resolution) + float(s.uncertainty))) <= 1e-15
        p, obar, cnt = metrics.reliability_curve(agree)
        assert np.isnan(obar[1:M]).all() and obar[0] == 0.3 and obar[M] == 0.8 and list(cnt) == [10, 0, 0, 0, 10]
        s = metrics.brier_scores(empty)
        assert all(np.isnan(float(v)) for v in s)
        c = metrics.contingency_scores(empty, 1)
        assert np.isnan(c.pod) and np.isnan(c.far) and np.isnan(c.csi) and int(c.hits) == 0
        assert np.isnan(metrics.roc_curve(empty).auc)
    with pytest.raises(ValueError):
        metrics.brier_scores(np.zeros((3, 5), dtype=np.int32))


# ---- the reference notices mistakes -----------------------------------------------------------------------------------------
def _mutant(kind, frames, y, thresholds, norm):
    """A copy of the statement (ensemble_exceed_reference.table) with one deliberate mistake."""
    frames, y = np.asarray(frames, dtype=np.float32), np.asarray(y, dtype=np.float32)
    n_steps, B, M, C, H, W = frames.shape
    thr = ref.thresholds_per_channel(thresholds, C)
    K = len(thr)
    v = ref.denorm(frames, norm, clamp=kind != "clamp_after")          # (a clamp after the comparison changes no count)
    q = y if kind == "truth_normalised" else ref.denorm(y, norm, clamp=kind != "clamp_after")
    out = np.zeros((B, n_steps, K, C, 2, M + 1), dtype=np.int32)
    for k in range(K):
        for c in range(C):
            th = thr[k][min(k, C - 1)] if kind == "thr_k_for_c" else thr[k][c]
            with np.errstate(invalid="ignore"):
                above = (v[:, :, :, c] >= th) if kind == "ge" else (v[:, :, :, c] > th)
                obs = (q[:, :, c] >= th) if kind == "ge" else (q[:, :, c] > th)
            nn = above.sum(2)                                               # [n, B, H, W]
            for i in range(n_steps):
                for b in range(B):
                    if kind == "swap":                                      # (the two axes have one extent at M = 1 only)
                        np.add.at(out[b, i, k, c], (nn[i, b].reshape(-1), obs[b, i].reshape(-1).astype(np.int64)), 1)
                    else:
                        np.add.at(out[b, i, k, c], (obs[b, i].reshape(-1).astype(np.int64), nn[i, b].reshape(-1)), 1)
    return out


def test_reference_catches_five_deliberate_mistakes():
    """>= for >, the o and n axes swapped, the truth left normalised, the clamp after the comparison, a threshold row indexed by
    k where c belongs: the unmutated copy equals the reference, and each mistake changes at least one count."""
    C = 3
    norm = dict(per_channel_norm(C))
    thr = thresholds_for(C)
    for m in (1, 3):
        frames, y = family_fields((2, 2, m, C, 5, 7), 900 + m)
        want = ref.table(frames, y, thr, norm)
        assert np.array_equal(_mutant("none", frames, y, thr, norm), want)
        kinds = ("ge", "truth_normalised", "clamp_after", "thr_k_for_c") + (("swap",) if m == 1 else ())
        for kind in kinds:
            got = _mutant(kind, frames, y, thr, norm)
            changed = int((got != want).sum())
            assert changed >= 1, (kind, m)
            assert got.sum() == want.sum()                                  # (every pixel is still counted once)

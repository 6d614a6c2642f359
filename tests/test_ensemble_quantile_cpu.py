"""CPU: the ensemble quantiles (lns_rollout_latent_ensemble_quantiles, lns_op_ensemble_quantiles, include/lns.h) are declared,
exported and bound, refuse bad arguments before any device work in the documented order, the kernel uses no scratch memory
-- and the fp32 statement the GPU tests hold it to (tests/ensemble_quantile_reference.py) has the properties a quantile /
exceedance reference must have, agrees with numpy.quantile in float64, and notices the mistakes an implementation can make."""
import copy
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from helpers import ROOT

QUANTILE_SYMBOLS = ("lns_rollout_latent_ensemble_quantiles", "lns_op_ensemble_quantiles")
_P = ctypes.c_void_p(0x1000)                          # stands for a device pointer; never dereferenced
_T = 5
FLOOR = 2e-7


def _ints(*v):
    return (ctypes.c_int * len(v))(*v)


def _norm(size=None, per_channel=0):
    from lns_amd import _lib
    s = _lib.LnsEvalSpec()
    s.size = ctypes.sizeof(_lib.LnsEvalSpec) if size is None else size
    s.per_channel = per_channel
    s.mean, s.std, s.eps = 0.0, 1.0, 1e-8
    return s


def _qspec(q=(0.05, 0.5, 0.95), n_thr=1, size=None, n_q=None):
    from lns_amd import _lib
    s = _lib.LnsEnsembleQuantileSpec()
    s.size = ctypes.sizeof(_lib.LnsEnsembleQuantileSpec) if size is None else size
    s.n_q, s.n_thr = (len(q) if n_q is None else n_q), n_thr
    for k, p in enumerate(q):
        s.q[k] = p
    return s


def test_quantile_symbols_are_declared_exported_and_bound():
    from lns_amd import _lib, dropin, engine, metrics
    _lib.build()
    src = open(os.path.join(ROOT, "include", "lns.h")).read()
    # the statement is in the header
    for text in ("key(x) = bits ^ (sign ? 0xFFFFFFFF : 0x80000000)", "h = p (M - 1);  lo = floor(h);  frac = (float)(h - lo)",
                 "d = v_(lo+1) - v_(lo);  t = frac * d;  Q_k = v_(lo) + t", "P_k = (float)#{m : v_m > thr[k][c]} / (float)M"):
        assert text in src, text
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(lns_[a-z0-9_]+)\s*\(", src))
    L = ctypes.CDLL(_lib.LIB_PATH)
    for s in QUANTILE_SYMBOLS:
        assert s in declared, "not declared in include/lns.h: " + s
        assert hasattr(L, s), "missing export: " + s
        assert s in _lib.SYMBOLS
        assert getattr(_lib.lib(), s).argtypes, "not bound in _lib.lib(): " + s
    assert re.search(r"#define\s+LNS_ABI_VERSION\s+2\b", src)         # additive: the ABI version stays
    assert "lns_ensemble_quantile_spec" in src
    assert ctypes.sizeof(_lib.LnsEnsembleQuantileSpec) == 16 + 8 * 8 + 8 * 8 * 4
    assert _lib.lib().lns_build_has(b"ensemble_quantiles") == 1
    assert _lib.lib().lns_build_has(b"ensemble_score") == 1
    assert engine.EnsembleQuantiles._fields == ("quantiles", "prob", "mean", "var", "z_last")
    assert engine.EnsembleScores._fields == ("rel_l2", "rmse", "spread", "crps", "seq", "rank", "mean", "var", "z_last")
    for owner, name in ((engine.Engine, "ensemble_quantiles"), (engine.Engine, "rollout_latent_ensemble_quantiles"),
                        (dropin.LatentDynamics, "predict_quantiles"), (metrics, "ensemble_quantiles")):
        assert callable(getattr(owner, name))


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
_QS = (-1, "qspec is null or its size field is not sizeof(lns_ensemble_quantile_spec)")
_NQ = (-1, "qspec: n_q and n_thr must be in 0 .. 8 and not both 0")
_PR = (-1, "qspec: every probability must be in [0, 1]")
_QO, _PO = (-1, "quant_out is null but n_q > 0"), (-1, "prob_out is null but n_thr > 0")
_MR = (-1, "ensemble quantiles need M in 1 .. 128")
_VM, _V2 = (-1, "var_out needs mean_out"), (-1, "var_out needs M >= 2")
_NORM = (-1, "norm: the size field is not sizeof(lns_eval_spec)")
_NPC = (-1, "norm: the per-channel form needs in_channels <= 8")
_CH = (-1, "thresholds need in_channels <= 8")
# (arguments of the call that differ from a valid one, expected (return code, message))
_REFUSALS = [
    (dict(), _PASSED), (dict(mean=None, var=None), _PASSED), (dict(var=None), _PASSED), (dict(last=_P), _PASSED),
    (dict(param=_P), _PASSED), (dict(ws=None), _PASSED), (dict(M=1, var=None), _PASSED), (dict(M=128), _PASSED),
    (dict(B=511, M=128), _PASSED), (dict(norm=None), _PASSED), (dict(norm="per_channel"), _PASSED),
    (dict(qs="only_q", prob=None), _PASSED), (dict(qs="only_thr", quant=None), _PASSED), (dict(qs="ends"), _PASSED),
    (dict(z=None), (-1, "z_in is null")),
    (dict(qs=None), _QS), (dict(qs="short"), _QS),
    (dict(qs="none"), _NQ), (dict(qs="nine_q"), _NQ), (dict(qs="neg_thr"), _NQ), (dict(qs="nine_thr"), _NQ),
    (dict(qs="nan"), _PR), (dict(qs="above"), _PR), (dict(qs="below"), _PR),
    (dict(quant=None), _QO), (dict(prob=None), _PO),
    (dict(B=0), _B), (dict(B=-1), _B), (dict(M=0), _M), (dict(M=-1), _M), (dict(T=0), _T0), (dict(T=-1), _T0),
    (dict(M=1), _V2), (dict(M=129), _MR), (dict(M=129, mean=None, var=None), _MR),
    (dict(mean=None), _VM),
    (dict(norm="short"), _NORM),
    # nine channels: the per-channel norm answers before the thresholds; quantiles alone with a scalar norm or none pass
    (dict(eng="wide", norm="per_channel"), _NPC), (dict(eng="wide", norm="per_channel", qs="only_q", prob=None), _NPC),
    (dict(eng="wide"), _CH), (dict(eng="wide", norm=None), _CH), (dict(eng="wide", qs="only_thr", quant=None), _CH),
    (dict(eng="wide", qs="only_q", prob=None), _PASSED), (dict(eng="wide", norm="short"), _NORM),
    (dict(k=_ints(0, 4, 3)), _KEEP_2_3), (dict(k=None), (-1, "keep_steps is null")),
    (dict(nk=0), _N_KEEP_1), (dict(nk=-1), _N_KEEP_1),
    (dict(B=512, M=128), _BATCH),
    (dict(eng="noprop"), _NO_MODEL),
    (dict(eng="cond"), (-1, "conditional propagator needs param")), (dict(eng="cond", param=_P), _PASSED),
    # two failing checks: arguments (in the order of the list above), then the batch, then the model, then param
    (dict(z=None, qs=None), (-1, "z_in is null")), (dict(qs=None, quant=None), _QS), (dict(qs="none", quant=None), _NQ),
    (dict(qs="nine_q", B=0), _NQ), (dict(qs="nan", quant=None), _PR), (dict(quant=None, prob=None), _QO), (dict(prob=None, B=0), _PO),
    (dict(B=0, M=0), _B), (dict(M=0, T=0), _M), (dict(T=0, M=129), _T0), (dict(M=129, mean=None), _MR),
    (dict(mean=None, norm="short"), _VM), (dict(norm="short", nk=0), _NORM), (dict(nk=0, k=None), _N_KEEP_1),
    (dict(k=_ints(0, 4, 3), B=512, M=128), _KEEP_2_3), (dict(norm="short", B=512, M=128), _NORM),
    (dict(qs=None, eng="noprop"), _QS), (dict(B=512, M=128, eng="noprop"), _BATCH),
    (dict(B=512, M=128, eng="cond"), _BATCH), (dict(M=129, eng="cond"), _MR), (dict(eng="noprop", param=_P), _NO_MODEL),
]


def _qspecs():
    return {"ok": _qspec(), "short": _qspec(size=8), "only_q": _qspec(n_thr=0), "only_thr": _qspec(q=(), n_thr=2),
            "ends": _qspec(q=(0.0, 1.0)), "none": _qspec(q=(), n_thr=0), "nine_q": _qspec(n_q=9), "neg_thr": _qspec(n_thr=-1),
            "nine_thr": _qspec(n_thr=9), "nan": _qspec(q=(0.5, float("nan"))), "above": _qspec(q=(0.5, 1.0000001)),
            "below": _qspec(q=(-1e-9, 0.5))}


def test_ensemble_quantiles_refuse_bad_arguments_without_a_device():
    """Every refusal is decided before the first HIP call (fake pointers, no device here), in the order arguments, batch
    (on B * M), model, param; a call that passes them all stops at the weights that were never finalised."""
    from lns_amd import _lib
    L = _lib.lib()
    engines = _engines()
    norms = {"ok": _norm(), "short": _norm(size=8), "per_channel": _norm(per_channel=1)}
    qspecs = _qspecs()
    assert L.lns_rollout_latent_ensemble_quantiles(None, _P, None, 2, 3, _T, _ints(0, 3, 4), 3, ctypes.byref(qspecs["ok"]), None, _P, _P,
                                                   _P, _P, None, _P, 1 << 30, None) == _lib.LNS_EINVAL
    for kw, (want_rc, want_msg) in _REFUSALS:
        a = dict(eng="full", z=_P, param=None, B=2, M=3, T=_T, k=_ints(0, 3, 4), nk=3, qs="ok", norm="ok", quant=_P, prob=_P,
                 mean=_P, var=_P, last=None, ws=_P)
        a.update(kw)
        h = engines[a["eng"]]._h
        qp = ctypes.byref(qspecs[a["qs"]]) if a["qs"] else None
        sp = ctypes.byref(norms[a["norm"]]) if a["norm"] else None
        rc = L.lns_rollout_latent_ensemble_quantiles(h, a["z"], a["param"], a["B"], a["M"], a["T"], a["k"], a["nk"], qp, sp, a["quant"],
                                                     a["prob"], a["mean"], a["var"], a["last"], a["ws"], 1 << 30, None)
        assert (rc, L.lns_last_error(h).decode()) == (want_rc, want_msg), kw


def test_ensemble_quantiles_op_refuses_bad_arguments_without_a_device():
    from lns_amd import _lib
    L = _lib.lib()
    ok, short, per_c = _norm(), _norm(size=8), _norm(per_channel=1)
    qs = _qspecs()

    def op(frames=_P, n=2, B=2, M=3, C=3, H=4, W=5, q="ok", norm=ok, quant=_P, prob=_P):
        return L.lns_op_ensemble_quantiles(frames, n, B, M, C, H, W, ctypes.byref(qs[q]) if q else None,
                                           ctypes.byref(norm) if norm is not None else None, quant, prob, None)
    for kw, word in ((dict(frames=None), "frames is null"), (dict(q=None), "qspec is null"), (dict(q="short"), "qspec is null"),
                     (dict(q="none"), "not both 0"), (dict(q="nine_q"), "0 .. 8"), (dict(q="nine_thr"), "0 .. 8"),
                     (dict(q="nan"), "probability"), (dict(q="above"), "probability"), (dict(q="below"), "probability"),
                     (dict(quant=None), "quant_out is null"), (dict(prob=None), "prob_out is null"),
                     (dict(norm=short), "spec is null or its size"), (dict(M=0), "M in 1 .. 128"), (dict(M=129), "M in 1 .. 128"),
                     (dict(n=0), "n >= 1"), (dict(B=0), "B in"), (dict(B=65536), "B in"), (dict(C=0), "C, H, W"), (dict(H=0), "C, H, W"),
                     (dict(W=-1), "C, H, W"), (dict(H=1 << 16, W=1 << 15), "H * W"), (dict(n=1 << 16, B=1 << 15, C=8), "n * B * C"),
                     (dict(C=9), "thresholds need C <= 8"), (dict(C=9, q="only_q", prob=None, norm=per_c), "C <= 8"),
                     # two failing checks: the order of the list above
                     (dict(frames=None, q=None), "frames is null"), (dict(q="nan", quant=None), "probability"),
                     (dict(prob=None, norm=short), "prob_out is null"), (dict(norm=short, M=0), "spec is null or its size"),
                     (dict(M=129, n=0), "M in 1 .. 128")):
        assert op(**kw) == _lib.LNS_EINVAL, kw
        msg = L.lns_create_error().decode()
        assert msg.startswith("ensemble_quantiles: ") and word in msg, (kw, msg)


def test_quantile_kernel_uses_no_scratch_and_spills_nothing():
    """tools/kernel_resources.py on the code object: 0 scratch bytes and 0 spilled registers for the quantile kernel (its
    member values live in LDS, not in a register array)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    from lns_amd import _lib
    res = kernel_resources.resources(_lib.LIB_PATH)
    k = [v for n, v in res.items() if "ensemble_quantile_kernel" in n]
    assert len(k) == 1
    assert k[0]["scratch"] == 0 and k[0]["vgpr_spill"] == 0 and k[0]["sgpr_spill"] == 0, k[0]


# ---- the statement itself (CPU) ---------------------------------------------------------------------------------------------
torch = pytest.importorskip("torch")

PROBS = (0.0, 0.05, 0.25, 1.0 / 3.0, 0.5, 0.95, 1.0)
THRESHOLDS = (-0.5, 0.25, (1.0, 0.0))
SCALAR = dict(mean=0.25, std=1.5)


def _frames(n, B, M, C, H, W, seed):
    g = torch.Generator()
    g.manual_seed(seed)
    return torch.randn((n, B, M, C, H, W), generator=g)


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def test_statement_against_numpy_quantile_in_float64():
    """statement32 on N(0,1) * 1.5 + 0.25 against numpy.quantile(method="linear") in float64 under the rule max(2e-7, 3 x own),
    own being torch.quantile's fp32 distance from the same float64 values; probabilities equal the float64 count / M rounded
    to fp32 exactly."""
    import ensemble_quantile_reference as ref
    for M in (2, 3, 7, 33, 128):
        frames = _frames(2, 2, M, 2, 5, 7, M)
        quant, prob = ref.statement32(frames, PROBS, THRESHOLDS, **SCALAR)
        q64, p64 = ref.quantiles64(frames, PROBS, THRESHOLDS, **SCALAR)
        own, _ = ref.own32(frames, PROBS, THRESHOLDS, **SCALAR)
        for what, err in (("rel-max", lambda a: float((a.double() - q64).abs().max() / q64.abs().max())),
                          ("rel-L2", lambda a: float((a.double() - q64).norm() / q64.norm()))):
            assert err(quant) <= max(FLOOR, 3.0 * err(own)), (M, what, err(quant), err(own))
        assert torch.equal(prob, p64.float())
        # and the package's stored-path statement is the same function of the same members
        from lns_amd import metrics
        mq, mp = metrics.ensemble_quantiles(frames.permute(1, 2, 0, 3, 4, 5).contiguous(), PROBS, THRESHOLDS, **SCALAR)
        assert _same(mq, quant) and _same(mp, prob)


def test_statement_order_statistics_and_monotonicity():
    import ensemble_quantile_reference as ref
    for M in (1, 2, 5, 11):
        frames = _frames(2, 3, M, 2, 4, 5, 10 + M)
        v = frames.permute(2, 1, 0, 3, 4, 5)                                   # [M, B, n, C, H, W]
        srt = v.sort(dim=0).values                                             # (no NaN, no zero of either sign: torch's order is the key's)
        # frac == 0: the order statistics themselves, bit for bit; p = k / (M - 1) is such a position
        probs = [k / (M - 1) for k in range(M)] if M > 1 else [0.0, 0.3, 1.0]
        quant = torch.cat([ref.statement32(frames, probs[i:i + 8])[0] for i in range(0, len(probs), 8)], 2)
        if M == 1:
            for k in range(3):
                assert _same(quant[:, :, k], v[0])                             # one member: every quantile is the member itself
        else:
            hit = [k for k in range(M) if probs[k] * (M - 1) == k]             # (k / (M - 1) * (M - 1) may round off k)
            assert len(hit) >= M - 2 and 0 in hit and M - 1 in hit
            for k in hit:
                assert _same(quant[:, :, k], srt[k]), (M, k)
        q01, _ = ref.statement32(frames, (0.0, 1.0))
        assert _same(q01[:, :, 0], v.amin(0)) and _same(q01[:, :, 1], v.amax(0))
        fine = [i / 40 for i in range(41)]
        for lo in range(0, 41, 8):
            qf, _ = ref.statement32(frames, fine[lo:lo + 8])
            assert bool((qf[:, :, 1:] >= qf[:, :, :-1]).all())                 # non-decreasing in p
        _, prob = ref.statement32(frames, (), (-1.0, -0.25, 0.0, 0.5, 2.0))
        assert bool((prob[:, :, 1:] <= prob[:, :, :-1]).all())                 # non-increasing in the threshold
        assert bool((prob >= 0).all()) and bool((prob <= 1).all())


def test_statement_total_order_of_zeros_infinities_and_nans():
    import ensemble_quantile_reference as ref
    nan = float("nan")
    v = torch.tensor([0.0, -0.0, float("inf"), -1.0, nan, float("-inf"), -nan, 1.0]).view(8, 1, 1, 1)
    s = ref.sort_members(v).view(-1)
    want = torch.tensor([-nan, float("-inf"), -1.0, -0.0, 0.0, 1.0, float("inf"), nan])
    assert torch.equal(torch.isnan(s), torch.isnan(want)) and torch.equal(torch.signbit(s), torch.signbit(want))
    assert torch.equal(s[1:7], want[1:7])
    assert torch.equal(ref.from_key(ref.to_key(v)).view(torch.int32), v.view(torch.int32))
    # a NaN member compares false against every threshold
    frames = v.view(1, 1, 8, 1, 1, 1)
    _, prob = ref.statement32(frames, (), (-2.0, 0.0, 0.5))
    assert prob.view(-1).tolist() == [5 / 8, 2 / 8, 2 / 8]


# Each mutant is one mistake an implementation can make; each must change some output on the inputs the tests use.
def _mutant(kind, frames, probs, thresholds, norm):
    import math
    import ensemble_quantile_reference as ref
    n, B, M, C, H, W = frames.shape
    if kind == "axes":                                   # members read with the [B][M] axes swapped
        frames = frames.reshape(n, M, B, C, H, W).permute(0, 2, 1, 3, 4, 5).contiguous()
    v = ref.members(frames, norm)
    pos = ref.positions(probs, M)
    if kind == "position":                               # p * M instead of p * (M - 1)
        pos = []
        for p in probs:
            h = min(float(p) * M, float(M - 1))
            lo = int(math.floor(h))
            pos.append((M - 1, 0.0) if lo >= M - 1 else (lo, float(np.float32(h - lo))))
    if kind == "lo":                                     # lo + 1 off by one: the upper neighbour is v_(lo+2)
        vs = ref.sort_members(v)
        rows = []
        for lo, frac in pos:
            hi = min(lo + 2, M - 1)
            rows.append(vs[lo] + torch.full_like(vs[lo], frac) * (vs[hi] - vs[lo]))
        quant = torch.stack(rows, 0)
    elif kind == "raw_sort":                             # sorted before the denormalisation instead of after it
        raw = ref.sort_members(frames.permute(2, 1, 0, 3, 4, 5).contiguous())
        vs = ref.denorm(raw.permute(2, 1, 0, 3, 4, 5), norm).permute(2, 1, 0, 3, 4, 5)
        quant = ref.interpolate32(vs, pos)
    else:
        quant = ref.interpolate32(ref.sort_members(v, descending=kind == "descending"), pos)
    prob = ref.exceed32(v, ref.thresholds_per_channel(thresholds, C), ge=kind == "ge")
    return quant.permute(1, 2, 0, 3, 4, 5).contiguous(), prob.permute(1, 2, 0, 3, 4, 5).contiguous()


def test_statement_catches_six_deliberate_mistakes():
    import ensemble_quantile_reference as ref
    n, B, M, C, H, W = 2, 2, 5, 2, 3, 4
    # quantised to 1/4 so that members tie at the thresholds; channel 1 has std < 0 (sorting before the map would reverse it)
    frames = (_frames(n, B, M, C, H, W, 77) * 4.0).round() / 4.0
    norm = dict(mean=[0.25, 0.5], std=[1.0, -2.0])
    thresholds = (0.25, (0.5, -1.0))
    want_q, want_p = ref.statement32(frames, PROBS, thresholds, **norm)
    same_q, same_p = _mutant(None, frames, PROBS, thresholds, norm)
    assert _same(same_q, want_q) and _same(same_p, want_p)                    # the unmutated composition is the statement
    assert bool((ref.members(frames, norm) == 0.25).any())                    # a tie at a threshold exists
    for kind, moves in (("position", "q"), ("lo", "q"), ("ge", "p"), ("descending", "q"), ("raw_sort", "q"), ("axes", "qp")):
        got_q, got_p = _mutant(kind, frames, PROBS, thresholds, norm)
        if "q" in moves:
            assert not _same(got_q, want_q), kind
        if "p" in moves:
            assert not _same(got_p, want_p), kind

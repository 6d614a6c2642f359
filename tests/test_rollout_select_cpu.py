"""CPU: the selected-step rollout (lns_rollout_select & co., include/lns.h) is declared, exported and bound, refuses bad
arguments before any device work, and `engine.normalize_keep_steps` resolves slices / ranges / lists as documented."""
import ctypes
import os
import re

import pytest

from helpers import ROOT

SELECT_SYMBOLS = ("lns_rollout_select_workspace_bytes", "lns_rollout_select", "lns_rollout_latent_select")


def test_select_symbols_are_declared_exported_and_bound():
    from lns_amd import _lib
    _lib.build()
    src = open(os.path.join(ROOT, "include", "lns.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(lns_[a-z0-9_]+)\s*\(", src))
    L = ctypes.CDLL(_lib.LIB_PATH)
    for s in SELECT_SYMBOLS:
        assert s in declared, "not declared in include/lns.h: " + s
        assert hasattr(L, s), "missing export: " + s
        assert s in _lib.SYMBOLS
        assert getattr(_lib.lib(), s).argtypes, "not bound in _lib.lib(): " + s
    assert re.search(r"#define\s+LNS_ABI_VERSION\s+2\b", src)         # additive: the ABI version stays


def test_build_has_rollout_select():
    from lns_amd import _lib
    assert _lib.lib().lns_build_has(b"rollout_select") == 1


def _engine():
    from lns_amd import config, engine
    return engine.Engine(engine.make_config(config.preset("ns2d_mini"), ae_prefix="vq_ae.", prop_prefix="propagator."))


def test_select_workspace_bytes_without_a_device():
    """Refusals are host-only.  The size itself needs the plans of lns_prepare (finalised weights): where lns_prepare
    answers, the selection workspace is its bytes plus a positive amount and lns_prepare's answer does not move; where
    it cannot (no device to finalise the weights on), the size function gives lns_prepare's status.
    (The sizes themselves are checked on the device build: tests/test_rollout_select_gpu.py.)"""
    from lns_amd import _lib
    L = _lib.lib()
    e = _engine()
    h = e._h
    n = ctypes.c_size_t(0)
    assert L.lns_rollout_select_workspace_bytes(None, 3, ctypes.byref(n)) == _lib.LNS_EINVAL
    assert L.lns_rollout_select_workspace_bytes(h, 0, ctypes.byref(n)) == _lib.LNS_EINVAL
    assert "B" in L.lns_last_error(h).decode()
    assert L.lns_rollout_select_workspace_bytes(h, 1 << 30, ctypes.byref(n)) == _lib.LNS_EINVAL
    assert "batch" in L.lns_last_error(h).decode()
    n0, n1, n2 = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    rc0 = L.lns_prepare(h, 3, ctypes.byref(n0))
    rc1 = L.lns_rollout_select_workspace_bytes(h, 3, ctypes.byref(n1))
    rc2 = L.lns_prepare(h, 3, ctypes.byref(n2))
    assert rc1 == rc0 and rc2 == rc0
    if rc0 == _lib.LNS_OK:
        assert n1.value > n0.value and n2.value == n0.value
    else:
        assert rc0 == _lib.LNS_ESTATE and n1.value == 0


def test_select_entry_points_refuse_bad_arguments_without_a_device():
    """Every LNS_EINVAL case is decided before the first HIP call: this runs on a machine without a GPU, with fake
    (never dereferenced) device pointers."""
    from lns_amd import _lib
    L = _lib.lib()
    e = _engine()
    h = e._h
    P = ctypes.c_void_p(0x1000)                       # stands for a device pointer
    keep = (ctypes.c_int * 3)(0, 3, 4)
    T = 5

    def err():
        return L.lns_last_error(h).decode()

    def sel(eng=h, x=P, B=3, T=T, k=keep, nk=3, out=P):
        return L.lns_rollout_select(eng, x, None, B, T, k, nk, out, None, P, 1 << 30, None)

    def lsel(eng=h, z=P, B=3, T=T, k=keep, nk=3, out=P):
        return L.lns_rollout_latent_select(eng, z, None, B, T, k, nk, out, None, P, 1 << 30, None)

    assert sel(eng=None) == _lib.LNS_EINVAL and lsel(eng=None) == _lib.LNS_EINVAL
    cases = ((dict(k=(ctypes.c_int * 3)(0, 4, 3)), "keep_steps"),        # unsorted
             (dict(k=(ctypes.c_int * 3)(0, 3, 3)), "keep_steps"),        # a duplicate
             (dict(k=(ctypes.c_int * 3)(-1, 3, 4)), "keep_steps"),       # -1
             (dict(k=(ctypes.c_int * 3)(0, 3, T)), "keep_steps"),        # T
             (dict(nk=0), "n_keep"), (dict(nk=-1), "n_keep"),
             (dict(k=None), "keep_steps"),                               # a null array
             (dict(B=0), "B"), (dict(T=0), "T"), (dict(out=None), "out"))
    for call, first, name in ((sel, "x", "x"), (lsel, "z", "z_in")):
        for kw, word in cases + ((({first: None}), name),):
            assert call(**kw) == _lib.LNS_EINVAL, (name, kw)
            assert word in err(), (name, kw, err())
    # the rule and the message of the evaluation calls' keep_steps
    assert sel(k=(ctypes.c_int * 3)(0, 4, 3)) == _lib.LNS_EINVAL
    assert err() == "keep_steps must be ascending steps in [0, 5): entry 2 is 3"


def test_keep_steps_normalisation():
    from lns_amd._lib import LnsError
    from lns_amd.engine import normalize_keep_steps as nk
    assert nk(slice(None, None, 5), 12) == [0, 5, 10]                  # the reference's y_hat[:, ::5]
    assert nk(slice(3, None, 4), 12) == [3, 7, 11]
    assert nk(slice(-2, None), 7) == [5, 6]
    assert nk(slice(None, 100), 3) == [0, 1, 2]                        # clipped like tensor indexing
    assert nk(range(1, 7, 2), 7) == [1, 3, 5]
    assert nk([0], 1) == [0] and nk((1, 4, 6), 7) == [1, 4, 6]
    import numpy as np
    assert nk(np.array([2, 3]), 7) == [2, 3] and all(type(v) is int for v in nk(np.array([2, 3]), 7))
    for bad, steps in (([], 7), (slice(5, 2), 7), (slice(None, None, -1), 7), ([3, 1], 7), ([1, 1], 7), ([-1], 7), ([7], 7),
                       (range(0, 9), 7), ([0.5], 7), ("ab", 7), (3, 7), (None, 7), ([0], 0)):
        with pytest.raises(LnsError):
            nk(bad, steps)


def test_keep_steps_of_latents_is_refused_before_anything_runs():
    """`keep_steps` with to_x=False says to slice the latent rollout (decided on the host: a CPU tensor gets the
    engine's no-fallback error first, so hand it the check directly)."""
    from lns_amd._lib import LnsError
    e = _engine()
    with pytest.raises(LnsError, match="slice the latent rollout"):
        e._keep_array(7, False, [0, 1])


# ---- the refusal matrix of the six rollout entry points and the three size queries -----------------------------------
# Every (return code, message) below was recorded from the library before the six entry points were merged into one call
# path; the order of the checks (argument checks, batch, eval_max_steps, LNS_ESTATE, param) is what the pairs pin.  None:
# the library set no message there before the merge, so only the code is pinned.
_T = 5
_P = ctypes.c_void_p(0x1000)                          # stands for a device pointer; never dereferenced


def _ints(*v):
    return (ctypes.c_int * len(v))(*v)


_CASES = {
    "valid": dict(),                                  # passes every refusal: stopped by the missing weights
    "param_given": dict(param=_P),
    "engine_null": dict(eng=None),
    "start_null": dict(start=None), "out_null": dict(out=None), "y_null": dict(y=None), "ws_null": dict(ws=None),
    "side_output_null": dict(side=None), "side_output_given": dict(side=_P),
    "B_0": dict(B=0), "B_negative": dict(B=-2), "B_huge": dict(B=1 << 30), "T_0": dict(T=0),
    "keep_unsorted": dict(k=_ints(0, 4, 3)), "keep_duplicate": dict(k=_ints(0, 3, 3)), "keep_minus_1": dict(k=_ints(-1, 3, 4)),
    "keep_T": dict(k=_ints(0, 3, _T)), "keep_null": dict(k=None), "n_keep_0": dict(nk=0), "n_keep_minus_1": dict(nk=-1),
    "frames_null": dict(frames=None), "frame_and_seq_null": dict(frame=None, seq=None), "frame_null": dict(frame=None),
    "spec_null": dict(spec=None), "spec_wrong_size": dict(spec="bad"),
    "t0_negative": dict(t0=-1), "t0_plus_T_past_T_total": dict(t0=4), "T_total_1": dict(Ttot=1),
    "past_eval_max_steps": dict(eng="max4"),
    "no_propagator": dict(eng="noprop"), "conditional_without_param": dict(eng="cond"),
    "conditional_with_param": dict(eng="cond", param=_P),
    # two failing checks: which one answers
    "start_null+no_propagator": dict(eng="noprop", start=None), "B_huge+no_propagator": dict(eng="noprop", B=1 << 30),
    "B_huge+past_eval_max_steps": dict(eng="max4", B=1 << 30), "past_eval_max_steps+no_propagator": dict(eng="noprop4"),
    "keep_unsorted+B_huge": dict(k=_ints(0, 4, 3), B=1 << 30), "n_keep_0+B_huge": dict(nk=0, B=1 << 30),
    "B_huge+conditional_without_param": dict(eng="cond", B=1 << 30), "T_0+conditional_without_param": dict(eng="cond", T=0),
    "spec_null+n_keep_minus_1": dict(spec=None, nk=-1), "out_null+B_0": dict(out=None, B=0), "y_null+B_0": dict(y=None, B=0),
    "to_x_0": dict(to_x=0), "to_x_0+B_huge": dict(to_x=0, B=1 << 30),
}
_NEEDS = {"out": ("lns_rollout", "lns_rollout_latent", "lns_rollout_select", "lns_rollout_latent_select"),
          "to_x": ("lns_rollout", "lns_rollout_latent"),
          "k": ("lns_rollout_eval", "lns_rollout_latent_eval", "lns_rollout_select", "lns_rollout_latent_select"),
          "nk": ("lns_rollout_eval", "lns_rollout_latent_eval", "lns_rollout_select", "lns_rollout_latent_select"),
          "y": ("lns_rollout_eval", "lns_rollout_latent_eval"), "frames": ("lns_rollout_eval", "lns_rollout_latent_eval"),
          "frame": ("lns_rollout_eval", "lns_rollout_latent_eval"), "seq": ("lns_rollout_eval", "lns_rollout_latent_eval"),
          "spec": ("lns_rollout_eval", "lns_rollout_latent_eval"), "t0": ("lns_rollout_latent_eval",), "Ttot": ("lns_rollout_latent_eval",)}
_SIZE_QUERIES = ("lns_prepare", "lns_rollout_eval_workspace_bytes", "lns_rollout_select_workspace_bytes")
_SIZE_CASES = {"valid": dict(), "engine_null": dict(eng=None), "B_0": dict(B=0), "B_negative": dict(B=-2), "B_huge": dict(B=1 << 30),
               "bytes_null": dict(n=None), "no_propagator": dict(eng="noprop"), "B_huge+no_propagator": dict(eng="noprop", B=1 << 30)}
_ENTRIES = ("lns_rollout", "lns_rollout_latent", "lns_rollout_eval", "lns_rollout_latent_eval", "lns_rollout_select",
            "lns_rollout_latent_select")


def _matrix_engines():
    from lns_amd import _lib, config, engine
    mini = config.preset("ns2d_mini")
    engines = {"full": _engine(), "max4": _engine(), "cond": engine.Engine(engine.make_config(
                   config.preset("twophase_cond"), ae_prefix="ae.", prop_prefix="propagator.")),
               "noprop": engine.Engine(engine.make_config(mini, prop_kind=_lib.LNS_PROP_NONE, ae_prefix="vq_ae.")),
               "noprop4": engine.Engine(engine.make_config(mini, prop_kind=_lib.LNS_PROP_NONE, ae_prefix="vq_ae."))}
    engines["max4"].set_option("eval_max_steps", 4)
    engines["noprop4"].set_option("eval_max_steps", 4)
    return engines


def _matrix_call(L, engines, entry, kw):
    """-> (rc, message or None) of one call; None: the call left the engine's last error alone."""
    from lns_amd import engine
    a = dict(eng="full", start=_P, param=None, y=_P, B=3, T=_T, t0=0, Ttot=_T, spec="ok", frame=_P, seq=_P, k=_ints(0, 3, 4),
             nk=3, frames=_P, out=_P, to_x=1, side=None, ws=_P, n=ctypes.c_size_t(0))
    a.update(kw)
    e = engines[a["eng"]] if a["eng"] else None
    h = e._h if e else None
    spec = engine.eval_spec(2, mean=0.37, std=1.9)
    if a["spec"] == "bad":
        spec.size = 8                                 # a struct of another version
    sp = ctypes.byref(spec) if a["spec"] else None
    if h:
        assert L.lns_set_option(h, b"no such option", 0) != 0          # a known last error: was it replaced?
        mark = L.lns_last_error(h)
    tail = (a["ws"], 1 << 30, None)
    if entry in _SIZE_QUERIES:
        rc = getattr(L, entry)(h, a["B"], ctypes.byref(a["n"]) if a["n"] is not None else None)
    elif entry in ("lns_rollout", "lns_rollout_latent"):
        rc = getattr(L, entry)(h, a["start"], a["param"], a["B"], a["T"], a["to_x"], a["out"], a["side"], *tail)
    elif entry == "lns_rollout_eval":
        rc = L.lns_rollout_eval(h, a["start"], a["param"], a["y"], a["B"], a["T"], sp, a["frame"], a["seq"], a["k"], a["nk"],
                                a["frames"], *tail)
    elif entry == "lns_rollout_latent_eval":
        rc = L.lns_rollout_latent_eval(h, a["start"], a["param"], a["y"], a["B"], a["T"], a["t0"], a["Ttot"], sp, a["frame"],
                                       a["seq"], a["k"], a["nk"], a["frames"], a["side"], *tail)
    else:
        rc = getattr(L, entry)(h, a["start"], a["param"], a["B"], a["T"], a["k"], a["nk"], a["out"], a["side"], *tail)
    msg = L.lns_last_error(h) if h else None
    return rc, (None if not h or msg == mark else msg.decode())


def _matrix_cases(entry):
    if entry in _SIZE_QUERIES:
        return list(_SIZE_CASES.items())
    return [(name, kw) for name, kw in _CASES.items() if all(entry in _NEEDS.get(k, _ENTRIES) for k in kw)]


_PASSED = (-3, "lns_finalize_weights must be called first")        # every refusal passed: no weights on this machine
_BATCH = (-1, "batch 1073741824 exceeds the maximum of 65535 trajectories per call")
_NO_MODEL = (-3, "rollout needs autoencoder and propagator")
_EINVAL = (-1, None)
_KEEP_2_3 = (-1, "keep_steps must be ascending steps in [0, 5): entry 2 is 3")
_MAX_STEPS = (-1, "5 steps exceed the option eval_max_steps = 4 (it sizes the evaluation workspace)")
_SPEC = (-1, "spec is null or its size field is not sizeof(lns_eval_spec)")
_N_KEEP_1 = (-1, "n_keep must be at least 1 (for no decoded step: lns_rollout with to_x = 0)")
_EXPECT = {
    "lns_rollout": {
        "valid": _PASSED, "param_given": _PASSED, "engine_null": _EINVAL, "start_null": _EINVAL, "out_null": _EINVAL,
        "ws_null": _PASSED, "side_output_null": _PASSED, "side_output_given": _PASSED, "B_0": _EINVAL, "B_negative": _EINVAL,
        "B_huge": _BATCH, "T_0": _EINVAL, "past_eval_max_steps": _PASSED, "no_propagator": _NO_MODEL,
        "conditional_without_param": (-1, "conditional model needs param"), "conditional_with_param": _PASSED,
        "start_null+no_propagator": _EINVAL, "B_huge+no_propagator": _BATCH, "B_huge+past_eval_max_steps": _BATCH,
        "past_eval_max_steps+no_propagator": _NO_MODEL, "B_huge+conditional_without_param": _BATCH,
        "T_0+conditional_without_param": _EINVAL, "out_null+B_0": _EINVAL, "to_x_0": _PASSED, "to_x_0+B_huge": _BATCH},
    "lns_rollout_latent": {
        "valid": _PASSED, "param_given": _PASSED, "engine_null": _EINVAL, "start_null": _EINVAL, "out_null": _EINVAL,
        "ws_null": _PASSED, "side_output_null": _PASSED, "side_output_given": _PASSED, "B_0": _EINVAL, "B_negative": _EINVAL,
        "B_huge": _BATCH, "T_0": _EINVAL, "past_eval_max_steps": _PASSED, "no_propagator": _NO_MODEL,
        "conditional_without_param": (-1, "conditional propagator needs param"), "conditional_with_param": _PASSED,
        "start_null+no_propagator": _EINVAL, "B_huge+no_propagator": _BATCH, "B_huge+past_eval_max_steps": _BATCH,
        "past_eval_max_steps+no_propagator": _NO_MODEL, "B_huge+conditional_without_param": _BATCH,
        "T_0+conditional_without_param": _EINVAL, "out_null+B_0": _EINVAL, "to_x_0": _PASSED, "to_x_0+B_huge": _BATCH},
    "lns_rollout_eval": {
        "valid": _PASSED, "param_given": _PASSED, "engine_null": _EINVAL, "start_null": (-1, "x is null"),
        "y_null": (-1, "y_true is null"), "ws_null": _PASSED, "side_output_null": _PASSED, "side_output_given": _PASSED,
        "B_0": (-1, "B must be positive"), "B_negative": (-1, "B must be positive"), "B_huge": _BATCH,
        "T_0": (-1, "T must be positive"), "keep_unsorted": _KEEP_2_3, "keep_duplicate": _KEEP_2_3,
        "keep_minus_1": (-1, "keep_steps must be ascending steps in [0, 5): entry 0 is -1"),
        "keep_T": (-1, "keep_steps must be ascending steps in [0, 5): entry 2 is 5"),
        "keep_null": (-1, "keep_steps is null but n_keep > 0"), "n_keep_0": _PASSED,
        "n_keep_minus_1": (-1, "n_keep is negative"), "frames_null": (-1, "frames_out is null but n_keep > 0"),
        "frame_and_seq_null": (-1, "frame_out and seq_out are both null"), "frame_null": _PASSED, "spec_null": _SPEC,
        "spec_wrong_size": _SPEC, "past_eval_max_steps": _MAX_STEPS, "no_propagator": _NO_MODEL,
        "conditional_without_param": (-1, "conditional model needs param"), "conditional_with_param": _PASSED,
        "start_null+no_propagator": (-1, "x is null"), "B_huge+no_propagator": _BATCH, "B_huge+past_eval_max_steps": _BATCH,
        "past_eval_max_steps+no_propagator": _MAX_STEPS, "keep_unsorted+B_huge": _KEEP_2_3, "n_keep_0+B_huge": _BATCH,
        "B_huge+conditional_without_param": _BATCH, "T_0+conditional_without_param": (-1, "T must be positive"),
        "spec_null+n_keep_minus_1": _SPEC, "y_null+B_0": (-1, "y_true is null")},
    "lns_rollout_latent_eval": {
        "valid": _PASSED, "param_given": _PASSED, "engine_null": _EINVAL, "start_null": (-1, "z_in is null"),
        "y_null": (-1, "y_true is null"), "ws_null": _PASSED, "side_output_null": _PASSED, "side_output_given": _PASSED,
        "B_0": (-1, "B must be positive"), "B_negative": (-1, "B must be positive"), "B_huge": _BATCH,
        "T_0": (-1, "T must be positive"), "keep_unsorted": _KEEP_2_3, "keep_duplicate": _KEEP_2_3,
        "keep_minus_1": (-1, "keep_steps must be ascending steps in [0, 5): entry 0 is -1"),
        "keep_T": (-1, "keep_steps must be ascending steps in [0, 5): entry 2 is 5"),
        "keep_null": (-1, "keep_steps is null but n_keep > 0"), "n_keep_0": _PASSED,
        "n_keep_minus_1": (-1, "n_keep is negative"), "frames_null": (-1, "frames_out is null but n_keep > 0"),
        "frame_and_seq_null": (-1, "frame_out and seq_out are both null"), "frame_null": _PASSED, "spec_null": _SPEC,
        "spec_wrong_size": _SPEC, "t0_negative": (-1, "t0 + T = -1 + 5 exceeds T_total = 5 (or t0 < 0)"),
        "t0_plus_T_past_T_total": (-1, "t0 + T = 4 + 5 exceeds T_total = 5 (or t0 < 0)"),
        "T_total_1": (-1, "t0 + T = 0 + 5 exceeds T_total = 1 (or t0 < 0)"), "past_eval_max_steps": _MAX_STEPS,
        "no_propagator": _NO_MODEL, "conditional_without_param": (-1, "conditional propagator needs param"),
        "conditional_with_param": _PASSED, "start_null+no_propagator": (-1, "z_in is null"), "B_huge+no_propagator": _BATCH,
        "B_huge+past_eval_max_steps": _BATCH, "past_eval_max_steps+no_propagator": _MAX_STEPS,
        "keep_unsorted+B_huge": _KEEP_2_3, "n_keep_0+B_huge": _BATCH, "B_huge+conditional_without_param": _BATCH,
        "T_0+conditional_without_param": (-1, "T must be positive"), "spec_null+n_keep_minus_1": _SPEC,
        "y_null+B_0": (-1, "y_true is null")},
    "lns_rollout_select": {
        "valid": _PASSED, "param_given": _PASSED, "engine_null": _EINVAL, "start_null": (-1, "x is null"),
        "out_null": (-1, "out is null"), "ws_null": _PASSED, "side_output_null": _PASSED, "side_output_given": _PASSED,
        "B_0": (-1, "B must be positive"), "B_negative": (-1, "B must be positive"), "B_huge": _BATCH,
        "T_0": (-1, "T must be positive"), "keep_unsorted": _KEEP_2_3, "keep_duplicate": _KEEP_2_3,
        "keep_minus_1": (-1, "keep_steps must be ascending steps in [0, 5): entry 0 is -1"),
        "keep_T": (-1, "keep_steps must be ascending steps in [0, 5): entry 2 is 5"), "keep_null": (-1, "keep_steps is null"),
        "n_keep_0": _N_KEEP_1, "n_keep_minus_1": _N_KEEP_1, "past_eval_max_steps": _PASSED, "no_propagator": _NO_MODEL,
        "conditional_without_param": (-1, "conditional model needs param"), "conditional_with_param": _PASSED,
        "start_null+no_propagator": (-1, "x is null"), "B_huge+no_propagator": _BATCH, "B_huge+past_eval_max_steps": _BATCH,
        "past_eval_max_steps+no_propagator": _NO_MODEL, "keep_unsorted+B_huge": _KEEP_2_3, "n_keep_0+B_huge": _N_KEEP_1,
        "B_huge+conditional_without_param": _BATCH, "T_0+conditional_without_param": (-1, "T must be positive"),
        "out_null+B_0": (-1, "out is null")},
    "lns_rollout_latent_select": {
        "valid": _PASSED, "param_given": _PASSED, "engine_null": _EINVAL, "start_null": (-1, "z_in is null"),
        "out_null": (-1, "out is null"), "ws_null": _PASSED, "side_output_null": _PASSED, "side_output_given": _PASSED,
        "B_0": (-1, "B must be positive"), "B_negative": (-1, "B must be positive"), "B_huge": _BATCH,
        "T_0": (-1, "T must be positive"), "keep_unsorted": _KEEP_2_3, "keep_duplicate": _KEEP_2_3,
        "keep_minus_1": (-1, "keep_steps must be ascending steps in [0, 5): entry 0 is -1"),
        "keep_T": (-1, "keep_steps must be ascending steps in [0, 5): entry 2 is 5"), "keep_null": (-1, "keep_steps is null"),
        "n_keep_0": _N_KEEP_1, "n_keep_minus_1": _N_KEEP_1, "past_eval_max_steps": _PASSED, "no_propagator": _NO_MODEL,
        "conditional_without_param": (-1, "conditional propagator needs param"), "conditional_with_param": _PASSED,
        "start_null+no_propagator": (-1, "z_in is null"), "B_huge+no_propagator": _BATCH, "B_huge+past_eval_max_steps": _BATCH,
        "past_eval_max_steps+no_propagator": _NO_MODEL, "keep_unsorted+B_huge": _KEEP_2_3, "n_keep_0+B_huge": _N_KEEP_1,
        "B_huge+conditional_without_param": _BATCH, "T_0+conditional_without_param": (-1, "T must be positive"),
        "out_null+B_0": (-1, "out is null")},
    "lns_prepare": {
        "valid": _PASSED, "engine_null": _EINVAL, "B_0": _EINVAL, "B_negative": _EINVAL, "B_huge": _BATCH,
        "bytes_null": _PASSED, "no_propagator": _PASSED, "B_huge+no_propagator": _BATCH},
    "lns_rollout_eval_workspace_bytes": {
        "valid": _PASSED, "engine_null": _EINVAL, "B_0": (-1, "B must be positive"), "B_negative": (-1, "B must be positive"),
        "B_huge": _BATCH, "bytes_null": _PASSED, "no_propagator": _NO_MODEL, "B_huge+no_propagator": _BATCH},
    "lns_rollout_select_workspace_bytes": {
        "valid": _PASSED, "engine_null": _EINVAL, "B_0": (-1, "B must be positive"), "B_negative": (-1, "B must be positive"),
        "B_huge": _BATCH, "bytes_null": _PASSED, "no_propagator": _NO_MODEL, "B_huge+no_propagator": _BATCH},
}


@pytest.mark.parametrize("entry", _ENTRIES + _SIZE_QUERIES)
def test_refusal_matrix(entry):
    """Return code and message of every refused call, and which of two failing checks answers, for each null pointer, B in
    {0, -2, 1 << 30}, T = 0, the keep_steps cases above, n_keep in {0, -1}, a bad spec, t0 + T > T_total, T_total >
    eval_max_steps, an engine without propagator and a conditional model without param.  Host only: fake pointers, no
    device; a call that passes every refusal stops at the weights that were never finalised."""
    from lns_amd import _lib
    L = _lib.lib()
    engines = _matrix_engines()
    cases = _matrix_cases(entry)
    assert [name for name, _ in cases] == list(_EXPECT[entry])
    for name, kw in cases:
        rc, msg = _matrix_call(L, engines, entry, kw)
        want_rc, want_msg = _EXPECT[entry][name]
        assert rc == want_rc, (entry, name, rc, msg)
        if want_msg is not None:
            assert msg == want_msg, (entry, name, msg)

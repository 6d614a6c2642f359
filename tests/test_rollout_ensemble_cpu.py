"""CPU: the ensemble rollout (lns_rollout_latent_ensemble, its size query and lns_op_ensemble_stats, include/lns.h) is
declared, exported and bound, refuses bad arguments before any device work in the documented order, and its reduction
kernel uses no scratch memory."""
import ctypes
import os
import re
import sys

from helpers import ROOT

ENSEMBLE_SYMBOLS = ("lns_rollout_ensemble_workspace_bytes", "lns_rollout_latent_ensemble", "lns_op_ensemble_stats")
_P = ctypes.c_void_p(0x1000)                          # stands for a device pointer; never dereferenced
_T = 5


def _ints(*v):
    return (ctypes.c_int * len(v))(*v)


def test_ensemble_symbols_are_declared_exported_and_bound():
    from lns_amd import _lib
    _lib.build()
    src = open(os.path.join(ROOT, "include", "lns.h")).read()
    assert "train_stage2_ns2d.py:211-212" in src and "train_stage2_ns2d.py:143-158" in src
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(lns_[a-z0-9_]+)\s*\(", src))
    L = ctypes.CDLL(_lib.LIB_PATH)
    for s in ENSEMBLE_SYMBOLS:
        assert s in declared, "not declared in include/lns.h: " + s
        assert hasattr(L, s), "missing export: " + s
        assert s in _lib.SYMBOLS
        assert getattr(_lib.lib(), s).argtypes, "not bound in _lib.lib(): " + s
    assert re.search(r"#define\s+LNS_ABI_VERSION\s+2\b", src)         # additive: the ABI version stays
    assert _lib.lib().lns_build_has(b"rollout_ensemble") == 1


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
_B, _M, _T0, _VAR = (-1, "B must be positive"), (-1, "M must be positive"), (-1, "T must be positive"), (-1, "var_out needs M >= 2")
# (arguments of the call that differ from a valid one, expected (return code, message))
_REFUSALS = [
    (dict(), _PASSED), (dict(var=None), _PASSED), (dict(M=1, var=None), _PASSED), (dict(last=_P), _PASSED),
    (dict(param=_P), _PASSED), (dict(ws=None), _PASSED), (dict(B=255, M=257), _PASSED),           # 65535 samples
    (dict(z=None), (-1, "z_in is null")), (dict(mean=None), (-1, "mean_out is null")),
    (dict(B=0), _B), (dict(B=-1), _B), (dict(M=0), _M), (dict(M=-1), _M), (dict(T=0), _T0), (dict(T=-1), _T0),
    (dict(M=1), _VAR),
    (dict(k=_ints(0, 4, 3)), _KEEP_2_3), (dict(k=_ints(0, 3, 3)), _KEEP_2_3),
    (dict(k=_ints(-1, 3, 4)), (-1, "keep_steps must be ascending steps in [0, 5): entry 0 is -1")),
    (dict(k=_ints(0, 3, _T)), (-1, "keep_steps must be ascending steps in [0, 5): entry 2 is 5")),
    (dict(k=None), (-1, "keep_steps is null")),
    (dict(nk=0), _N_KEEP_1), (dict(nk=-1), _N_KEEP_1),
    (dict(B=256, M=256), _BATCH),
    (dict(B=1 << 30, M=1 << 30), (-1, "batch 2147483647 exceeds the maximum of 65535 trajectories per call")),
    (dict(eng="noprop"), _NO_MODEL),
    (dict(eng="cond"), (-1, "conditional propagator needs param")), (dict(eng="cond", param=_P), _PASSED),
    # two failing checks: arguments, then the batch, then the model, then param
    (dict(z=None, mean=None), (-1, "z_in is null")), (dict(mean=None, B=0), (-1, "mean_out is null")),
    (dict(B=0, M=0), _B), (dict(M=0, T=0), _M), (dict(T=0, M=1), _T0), (dict(M=1, k=_ints(0, 4, 3)), _VAR),
    (dict(nk=0, k=None), _N_KEEP_1), (dict(k=_ints(0, 4, 3), B=256, M=256), _KEEP_2_3),
    (dict(z=None, eng="noprop"), (-1, "z_in is null")), (dict(B=256, M=256, eng="noprop"), _BATCH),
    (dict(B=256, M=256, eng="cond"), _BATCH), (dict(T=0, eng="cond"), _T0),
]


def test_ensemble_entry_point_refuses_bad_arguments_without_a_device():
    """Every refusal is decided before the first HIP call (fake pointers, no device here), in the order arguments, batch
    (on B * M), model, param; a call that passes them all stops at the weights that were never finalised."""
    from lns_amd import _lib
    L = _lib.lib()
    engines = _engines()
    assert L.lns_rollout_latent_ensemble(None, _P, None, 2, 3, _T, _ints(0, 3, 4), 3, _P, _P, None, _P, 1 << 30, None) == _lib.LNS_EINVAL
    for kw, (want_rc, want_msg) in _REFUSALS:
        a = dict(eng="full", z=_P, param=None, B=2, M=3, T=_T, k=_ints(0, 3, 4), nk=3, mean=_P, var=_P, last=None, ws=_P)
        a.update(kw)
        h = engines[a["eng"]]._h
        rc = L.lns_rollout_latent_ensemble(h, a["z"], a["param"], a["B"], a["M"], a["T"], a["k"], a["nk"], a["mean"], a["var"],
                                           a["last"], a["ws"], 1 << 30, None)
        assert (rc, L.lns_last_error(h).decode()) == (want_rc, want_msg), kw


def test_ensemble_stats_op_refuses_bad_arguments_without_a_device():
    from lns_amd import _lib
    L = _lib.lib()

    def op(frames=_P, B=2, M=3, per=5, mean=_P, var=_P):
        return L.lns_op_ensemble_stats(frames, B, M, per, mean, var, None)
    for kw, word in ((dict(frames=None), "null"), (dict(mean=None), "null"), (dict(B=0), "B in"), (dict(B=65536), "B in"),
                     (dict(M=0), "M in"), (dict(per=0), "per in"), (dict(per=(1 << 40) + 1), "per in"), (dict(M=1), "var needs M >= 2")):
        assert op(**kw) == _lib.LNS_EINVAL, kw
        assert word in L.lns_create_error().decode(), (kw, L.lns_create_error())


def test_ensemble_workspace_bytes_without_a_device():
    """The size query refuses on the host and otherwise follows lns_prepare(B * M)'s status (no device here: no finalised
    weights, so no plans to size); it does not move lns_prepare's answer.  (The size itself: tests/test_rollout_ensemble_gpu.py.)"""
    from lns_amd import _lib
    L = _lib.lib()
    engines = _engines()
    h = engines["full"]._h
    n = ctypes.c_size_t(0)

    def err():
        return L.lns_last_error(h).decode()
    assert L.lns_rollout_ensemble_workspace_bytes(None, 2, 3, ctypes.byref(n)) == _lib.LNS_EINVAL
    assert L.lns_rollout_ensemble_workspace_bytes(h, 0, 3, ctypes.byref(n)) == _lib.LNS_EINVAL and err() == "B must be positive"
    assert L.lns_rollout_ensemble_workspace_bytes(h, 2, 0, ctypes.byref(n)) == _lib.LNS_EINVAL and err() == "M must be positive"
    assert L.lns_rollout_ensemble_workspace_bytes(h, 256, 256, ctypes.byref(n)) == _lib.LNS_EINVAL and err() == _BATCH[1]
    hn = engines["noprop"]._h
    assert L.lns_rollout_ensemble_workspace_bytes(hn, 2, 3, ctypes.byref(n)) == _lib.LNS_ESTATE
    assert L.lns_last_error(hn).decode() == _NO_MODEL[1]
    n0, n1, n2 = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    rc0 = L.lns_prepare(h, 6, ctypes.byref(n0))
    rc1 = L.lns_rollout_ensemble_workspace_bytes(h, 2, 3, ctypes.byref(n1))
    rc2 = L.lns_prepare(h, 6, ctypes.byref(n2))
    assert rc1 == rc0 and rc2 == rc0
    if rc0 == _lib.LNS_OK:
        assert n1.value > n0.value and n2.value == n0.value
    else:
        assert rc0 == _lib.LNS_ESTATE and n1.value == 0


def test_ensemble_stats_kernel_uses_no_scratch_and_spills_nothing():
    """tools/kernel_resources.py on the code object: 0 scratch bytes and 0 spilled registers (a memory-bound elementwise
    kernel: anything else would be a regression)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    from lns_amd import _lib
    res = kernel_resources.resources(_lib.LIB_PATH)
    k = [v for n, v in res.items() if "ensemble_stats_kernel" in n]
    assert len(k) == 1
    assert k[0]["scratch"] == 0 and k[0]["vgpr_spill"] == 0 and k[0]["sgpr_spill"] == 0 and k[0]["vgpr"] <= 64, k[0]

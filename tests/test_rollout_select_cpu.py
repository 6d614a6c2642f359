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
        e._select_common(None, 7, False, None, [0, 1])

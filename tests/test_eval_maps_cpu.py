"""CPU: the host side of the time maps (include/lns.h "time maps"): exports and bindings, the statement against independent
float64 reductions under the project's rule, the statement fed in chunks, the refusals of the two streaming entry points and
of the op (host only, fake pointers), the map_steps argument, and the resources of the built kernels."""
import ctypes
import os
import sys

import pytest
import torch

import test_eval_stats_cpu as tsc
import time_maps_reference as tm
from helpers import ROOT

NEW = ("lns_rollout_eval_maps_workspace_bytes", "lns_rollout_eval_maps", "lns_rollout_latent_eval_maps",
       "lns_time_maps_state_bytes", "lns_op_time_maps")
FLOOR = 2e-7


def test_symbols_are_declared_exported_and_bound():
    from lns_amd import _lib, dropin, engine, metrics
    header = open(os.path.join(ROOT, "include", "lns.h")).read()
    L = _lib.lib()
    for sym in NEW:
        assert "int %s(" % sym in header, sym
        assert sym in _lib.SYMBOLS and hasattr(L, sym), sym
        assert getattr(L, sym).argtypes is not None, sym
    assert L.lns_build_has(b"eval_maps") == 1
    assert '"eval_maps"' in header and "#define LNS_TIME_MAPS 7" in header
    assert _lib.LNS_TIME_MAPS == 7
    # six 4-byte fields, seven pointers
    assert ctypes.sizeof(_lib.LnsEvalSelect) == 24 + 7 * ctypes.sizeof(ctypes.c_void_p)
    assert [n for n, _ in _lib.LnsEvalSelect._fields_] == [
        "size", "n_spec", "n_stats", "map_from", "map_every", "reserved", "spectrum_steps_host", "spectra_out",
        "stats_steps_host", "hspec", "stats_out", "hist_out", "maps_out"]
    for name in ("rollout_eval_maps", "rollout_latent_eval_maps", "time_maps"):
        assert callable(getattr(engine.Engine, name)), name
    assert callable(metrics.time_maps) and callable(metrics.temporal_correlation) and callable(metrics.rmse_map)
    assert metrics.TIME_MAPS == tm.NAMES and len(metrics.TIME_MAPS) == 7
    assert callable(dropin.LatentDynamics.validate_maps)
    assert engine.EvalMaps._fields == engine.EvalStats._fields + ("maps", "map_steps")
    assert engine.EvalMapsChunk._fields == engine.EvalMaps._fields + ("z_last",)
    n = ctypes.c_size_t(0)
    assert L.lns_time_maps_state_bytes(3, 2, 5, 7, ctypes.byref(n)) == 0 and n.value == (3 * 2 * 5 * 7 * 52 + 255) // 256 * 256
    assert L.lns_time_maps_state_bytes(64, 3, 128, 128, ctypes.byref(n)) == 0 and n.value == 64 * 3 * 128 * 128 * 52
    assert L.lns_time_maps_state_bytes(0, 2, 5, 7, ctypes.byref(n)) == _lib.LNS_EINVAL


def _errs(a, want):
    d = a.double() - want
    return float(d.abs().max() / want.abs().max()), float(d.norm() / want.norm())


def rule(ours, own, want, what):
    """max(2e-7, 3 x own) against float64, in both measures -> the larger ratio ours / bound.  A map that is exactly zero in
    float64 (the second moments over one step) must be exactly zero."""
    if float(want.abs().max()) == 0.0:
        assert float(ours.abs().max()) == 0.0, what
        return 0.0
    o, w = _errs(ours, want), _errs(own, want)
    ratios = [a / max(FLOOR, 3.0 * b) for a, b in zip(o, w)]
    print("%s: rel-max %.3e (own %.3e) rel-L2 %.3e (own %.3e) -> %.3f %.3f of the bound" % (what, o[0], w[0], o[1], w[1], ratios[0], ratios[1]))
    assert o[0] <= max(FLOOR, 3.0 * w[0]) and o[1] <= max(FLOOR, 3.0 * w[1]), (what, o, w)
    return max(ratios)


@pytest.mark.parametrize("family", tm.FAMILIES)
def test_the_statement_is_admissible_under_the_rule(family):
    """The statement (float64 sums of fp32 fields shifted by the truth's first frame) against independent float64 reductions,
    under max(2e-7, 3 x own) with torch's fp32 reductions as `own`, on a 17x16 plane for n = 1 .. 1024.  The error does not
    grow with n: it is the single rounding of each result to fp32."""
    g = torch.Generator().manual_seed(11)
    worst = 0.0
    for n in (1, 2, 5, 64, 1024):
        p, q = tm.family(family, (1, n, 2, 17, 16), g)
        ours, own, want = tm.statement64(p, q), tm.own32(p, q), tm.direct64(p, q)
        assert ours.dtype == torch.float32 and ours.shape == (1, 2, 7, 17, 16)
        if n == 1:
            assert bool((ours[:, :, 2:5] == 0).all())
        for k, name in enumerate(tm.NAMES):
            worst = max(worst, rule(ours[:, :, k], own[:, :, k], want[:, :, k], "%s n=%d %s" % (family, n, name)))
    print("%s: statement / bound = %.3f" % (family, worst))


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_the_statement_in_chunks_has_the_bits_of_the_statement_at_once():
    g = torch.Generator().manual_seed(3)
    T = 8
    p, q = tm.family("drift", (2, T, 2, 3, 5), g)
    norm = dict(mean=[0.4, -0.2], std=[2.1, 1.7], zero_wall_channels=(0,), clamp_channels=(1,), clamp=(-1.0, 1.5))
    for sel in ((0, 1), (1, 2), (3, 2), (4, 3), (7, 1), (2, 5)):
        one = tm.statement64(p, q, *sel, **norm)
        for cut in range(1, T):                               # split at any step
            assert _bits(tm.statement64(p, q, *sel, chunks=[cut, T - cut], **norm), one), (sel, cut)
        # 3 + 1 + 4: with (4, 3) the first two chunks select nothing and map_from lies in the last; with (3, 2) in the second
        assert _bits(tm.statement64(p, q, *sel, chunks=[3, 1, 4], **norm), one), sel
        assert _bits(tm.statement64(p, q, *sel, chunks=[1] * T, **norm), one), sel
    assert tm.selected(3, 4, 3, 0) == [] and tm.selected(1, 4, 3, 3) == [] and tm.selected(4, 4, 3, 4) == [4, 7]
    assert tm.selected(1, 3, 2, 3) == [3]


# ---- refusals (host only) ---------------------------------------------------------------------------------------------
_P, _T, _ints, _hspec = tsc._P, tsc._T, tsc._ints, tsc._hspec


def _select(a):
    from lns_amd import _lib
    q = _lib.LnsEvalSelect()
    q.size = ctypes.sizeof(_lib.LnsEvalSelect) if a["size"] is None else a["size"]
    q.n_spec, q.n_stats, q.map_from, q.map_every = a["ns"], a["nst"], a["mfrom"], a["mevery"]
    if a["sel"] is not None:
        q.spectrum_steps_host = a["sel"]
    if a["st"] is not None:
        q.stats_steps_host = a["st"]
    if a["hs"] is not None:
        q.hspec = ctypes.pointer(a["hs"])
    q.spectra_out, q.stats_out, q.hist_out, q.maps_out = a["spectra"], a["stats"], a["hist"], a["maps"]
    return q


def _call(L, engines, entry, kw):
    from lns_amd import engine
    a = dict(eng="full", start=_P, y=_P, B=3, T=_T, t0=0, Ttot=_T, spec="ok", frame=_P, seq=_P, k=_ints(0, 3, 4), nk=3,
             frames=_P, sel=_ints(0, 3, 4), ns=3, spectra=_P, st=_ints(1, 2, 4), nst=3, hs=_hspec(), stats=_P, hist=_P,
             size=None, mfrom=1, mevery=2, maps=_P, q="given")
    a.update(kw)
    e = engines[a["eng"]]
    sp = engine.eval_spec(2, mean=0.37, std=1.9)
    if a["spec"] == "bad":
        sp.size = 8
    assert L.lns_set_option(e._h, b"no such option", 0) != 0           # a known last error: was it replaced?
    mark = L.lns_last_error(e._h)
    q = _select(a)
    head = (e._h, a["start"], None, a["y"], a["B"], a["T"])
    mid = (ctypes.byref(sp), a["frame"], a["seq"], a["k"], a["nk"], a["frames"])
    tail = (_P, 1 << 40, None, ctypes.byref(q) if a["q"] == "given" else None)
    if entry == "lns_rollout_eval_maps":
        rc = L.lns_rollout_eval_maps(*head, *mid, *tail)
    else:
        rc = L.lns_rollout_latent_eval_maps(*head, a["t0"], a["Ttot"], *mid, None, *tail)
    msg = L.lns_last_error(e._h)
    return rc, (None if msg == mark else msg.decode())


_PASSED, _BATCH, _PLANE, _EDGES = tsc._PASSED, tsc._BATCH, tsc._PLANE, tsc._EDGES
_SIZE = (-1, "sel is null or its size field is not sizeof(lns_eval_select)")
_FROM = "map_from must be a step in [0, 5), got %d"
_CASES = {
    "valid": (dict(), _PASSED),
    "every_step": (dict(mfrom=0, mevery=1), _PASSED),
    "last_step_only": (dict(mfrom=4, mevery=1000), _PASSED),
    "maps_only": (dict(sel=None, ns=0, spectra=None, st=None, nst=0, hs=None, stats=None, hist=None), _PASSED),
    "no_spectra": (dict(sel=None, ns=0, spectra=None), _PASSED),
    "no_stats": (dict(st=None, nst=0, hs=None, stats=None, hist=None), _PASSED),
    "no_stats_pointers_ignored": (dict(nst=0, stats=None), _PASSED),
    "no_kept_frames": (dict(k=None, nk=0, frames=None), _PASSED),
    "big_plane_without_spectra": (dict(eng="big", sel=None, ns=0, spectra=None), _PASSED),
    "sel_null": (dict(q=None), _SIZE),
    "size_0": (dict(size=0), _SIZE),
    "size_short": (dict(size=72), _SIZE),
    "size_long": (dict(size=88), _SIZE),
    "maps_null": (dict(maps=None), (-1, "maps_out is null")),
    "every_0": (dict(mevery=0), (-1, "map_every must be at least 1")),
    "every_negative": (dict(mevery=-3), (-1, "map_every must be at least 1")),
    "from_negative": (dict(mfrom=-1), (-1, _FROM % -1)),
    "from_T_total": (dict(mfrom=5), (-1, _FROM % 5)),
    # the existing refusals keep their code, message and place ...
    "start_null": (dict(start=None), (-1, None)),
    "y_null": (dict(y=None), (-1, "y_true is null")),
    "spec_bad": (dict(spec="bad"), (-1, "spec is null or its size field is not sizeof(lns_eval_spec)")),
    "keep_unsorted": (dict(k=_ints(0, 4, 3)), (-1, "keep_steps must be ascending steps in [0, 5): entry 2 is 3")),
    "spectra_null": (dict(spectra=None), (-1, "spectra_out is null")),
    "n_spec_negative": (dict(ns=-1), (-1, "n_spec must be at least 1")),
    "plane_unsupported": (dict(eng="big"), _PLANE),
    "stats_null": (dict(stats=None), (-1, "stats_out is null")),
    "n_stats_negative": (dict(nst=-1), (-1, "n_stats must be at least 1")),
    "stats_steps_T": (dict(st=_ints(0, 3, 5)), (-1, tsc._STEPS % (2, 5))),
    "hist_without_hspec": (dict(hs=None), (-1, "hist_out needs a histogram description (hspec is null)")),
    "edge_equal": (dict(hs=_hspec(edges={1: (0.5, 0.5)})), _EDGES),
    "B_huge": (dict(B=1 << 30), _BATCH),
    "past_eval_max_steps": (dict(eng="max4"), (-1, "5 steps exceed the option eval_max_steps = 4 (it sizes the evaluation workspace)")),
    "no_propagator": (dict(eng="noprop"), (-3, "rollout needs autoencoder and propagator")),
    # ... and which of two failing checks answers: the existing calls', the two selections', the new ones in the written
    # order, then the batch check and the rest
    "maps_null+keep_unsorted": (dict(maps=None, k=_ints(0, 4, 3)), (-1, "keep_steps must be ascending steps in [0, 5): entry 2 is 3")),
    "maps_null+spectra_null": (dict(maps=None, spectra=None), (-1, "spectra_out is null")),
    "maps_null+stats_null": (dict(maps=None, stats=None), (-1, "stats_out is null")),
    "size+y_null": (dict(size=8, y=None), (-1, "y_true is null")),
    "size+spectra_null": (dict(size=8, spectra=None), _SIZE),          # an unreadable struct: its selections count as absent
    "size+maps_null": (dict(size=8, maps=None), _SIZE),
    "maps_null+every_0": (dict(maps=None, mevery=0), (-1, "maps_out is null")),
    "every_0+from_T_total": (dict(mevery=0, mfrom=5), (-1, "map_every must be at least 1")),
    "from_T_total+B_huge": (dict(mfrom=5, B=1 << 30), (-1, _FROM % 5)),
    "every_0+past_eval_max_steps": (dict(mevery=0, eng="max4"), (-1, "map_every must be at least 1")),
    "maps_null+no_propagator": (dict(maps=None, eng="noprop"), (-1, "maps_out is null")),
}


@pytest.mark.parametrize("entry", ["lns_rollout_eval_maps", "lns_rollout_latent_eval_maps"])
def test_refusal_matrix_of_the_maps_calls(entry):
    from lns_amd import _lib
    L = _lib.lib()
    engines = tsc._engines()
    for name, (kw, (want_rc, want_msg)) in _CASES.items():
        rc, msg = _call(L, engines, entry, kw)
        if name == "start_null":
            want_msg = "x is null" if entry == "lns_rollout_eval_maps" else "z_in is null"
        assert rc == want_rc, (entry, name, rc, msg)
        assert msg == want_msg, (entry, name, msg)
    # the chunked form: the selections are relative to the chunk (T), map_from to the horizon (T_total)
    chunk = dict(T=2, t0=3, k=_ints(0), nk=1, sel=_ints(1), ns=1, st=_ints(0, 1), nst=2)
    assert _call(L, engines, "lns_rollout_latent_eval_maps", dict(chunk, mfrom=4)) == _PASSED
    assert _call(L, engines, "lns_rollout_latent_eval_maps", dict(chunk, mfrom=0, mevery=7)) == _PASSED
    assert _call(L, engines, "lns_rollout_latent_eval_maps", dict(chunk, mfrom=5)) == (-1, _FROM % 5)
    # the size query refuses what lns_rollout_eval_workspace_bytes refuses
    n = ctypes.c_size_t(0)
    for eng, B in (("full", 0), ("full", 1 << 30), ("noprop", 3)):
        h = engines[eng]._h
        assert L.lns_rollout_eval_maps_workspace_bytes(h, B, ctypes.byref(n)) == L.lns_rollout_eval_workspace_bytes(h, B, ctypes.byref(n)) != 0


def test_refusals_of_the_op():
    from lns_amd import _lib, engine
    L = _lib.lib()
    spec = engine.eval_spec(2)
    bad = engine.eval_spec(2)
    bad.size = 8
    per9 = engine.eval_spec(8, mean=[0.0] * 8, std=[1.0] * 8)
    need = 52 * 1 * 2 * 4 * 4
    need = (need + 255) // 256 * 256

    def run(a=_P, g=_P, dims=(1, 3, 2, 4, 4), sp=spec, mfrom=0, mevery=1, o=_P, st=_P, nbytes=need):
        rc = L.lns_op_time_maps(a, g, *dims, ctypes.byref(sp) if sp is not None else None, mfrom, mevery, o, st, nbytes, None)
        return rc, L.lns_create_error().decode()
    for kw, text in ((dict(a=None), "null"), (dict(g=None), "null"), (dict(o=None), "null"), (dict(sp=None), "spec is null"),
                     (dict(sp=bad), "size field"), (dict(dims=(0, 3, 2, 4, 4)), "B, C, H, W >= 1"),
                     (dict(dims=(1, 0, 2, 4, 4)), "T >= 1"), (dict(dims=(1, 3, 2, 4, 0)), "B, C, H, W >= 1"),
                     (dict(dims=(1 << 16, 3, 2, 4, 4)), "B <= 65535"), (dict(dims=(1, 3, 9, 4, 4), sp=per9), "C <= 8"),
                     (dict(mevery=0), "map_every"), (dict(mfrom=-1), "map_from"), (dict(mfrom=3), "map_from"),
                     (dict(st=None), "state is null"), (dict(st=ctypes.c_void_p(0x1004)), "8-byte aligned")):
        rc, msg = run(**kw)
        assert rc == _lib.LNS_EINVAL and text in msg, (kw, rc, msg)
    rc, msg = run(nbytes=need - 1)
    assert rc == _lib.LNS_ENOMEM and "state too small: need %d bytes, got %d" % (need, need - 1) in msg


def test_map_steps_parsing_needs_no_device():
    import numpy as np
    from lns_amd import dropin, engine, metrics
    f = engine.normalize_map_steps
    assert f(None) == (0, 1)
    assert f(slice(None)) == (0, 1) and f(slice(8, None)) == (8, 1) and f(slice(None, None, 4)) == (0, 4)
    assert f(slice(16, None, 8)) == (16, 8) and f((16, 8)) == (16, 8) and f([0, 1]) == (0, 1)
    assert f((np.int64(3), np.int32(2))) == (3, 2)
    for bad in (slice(0, 10), slice(0, 10, 2), slice(-1, None), slice(0, None, 0), slice(0, None, -1), (0,), (0, 1, 2), (0, 0),
                (-1, 1), (0.0, 1), (0, 1.5), (True, 1), "0:1", 5, range(0, 10, 2), [0, 2, 4], slice(None, None, 2.0)):
        with pytest.raises(ValueError, match="map_steps"):
            f(bad)
    # the public entries raise it before they look at their tensors
    with pytest.raises(ValueError, match="map_steps"):
        metrics.time_maps(None, None, map_steps=[0, 2, 4])
    with pytest.raises(ValueError, match="map_steps"):
        engine.Engine.rollout_eval_maps(None, None, None, map_steps=5)
    with pytest.raises(ValueError, match="map_steps"):
        engine.Engine.rollout_latent_eval_maps(None, None, None, map_steps=(0, 0))
    with pytest.raises(ValueError, match="map_steps"):
        dropin.LatentDynamics.validate_maps(None, None, None, map_steps=slice(0, 4))


def test_derived_maps():
    from lns_amd import metrics
    maps = torch.zeros((1, 1, 7, 1, 3))
    maps[0, 0, 2] = torch.tensor([4.0, 0.0, 1.0])
    maps[0, 0, 3] = torch.tensor([9.0, 2.0, 0.0])
    maps[0, 0, 4] = torch.tensor([-3.0, 0.0, 0.0])
    maps[0, 0, 5] = torch.tensor([16.0, 0.25, 0.0])
    assert metrics.temporal_correlation(maps).tolist() == [[[[-0.5, 0.0, 0.0]]]]
    assert metrics.rmse_map(maps).tolist() == [[[[4.0, 0.5, 0.0]]]]


def test_kernels_use_no_scratch_and_spill_nothing():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    from lns_amd import _lib
    res = {k: v for k, v in kernel_resources.resources(_lib.LIB_PATH).items() if "time_maps" in k}
    kinds = sorted(set(n.split("time_maps_")[1].split("_kernel")[0] for n in res))
    assert kinds == ["finish", "group", "stored"] and len(res) == 5, sorted(res)   # group / stored: one and four pixels a thread
    for name, r in res.items():
        print(name, r)
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
        assert r["lds"] == 0, (name, r)                                 # a thread owns its pixels: nothing is shared
        assert r["vgpr"] + r["agpr"] <= 128, (name, r)                  # 256 threads: at least four blocks per CU fit the register file

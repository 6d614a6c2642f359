"""CPU: the host side of the field statistics (include/lns.h "field statistics"): exports and bindings, the float64 reference
against the real reference's recorded values, the bin rule on edge values, the refusals of the two streaming entry points
(host only, fake pointers), correlation_time, and the resources of the built kernels."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import field_stats_reference as fr
from helpers import ROOT

NEW = ("lns_rollout_eval_stats", "lns_rollout_latent_eval_stats", "lns_op_field_stats")


def test_symbols_are_declared_exported_and_bound():
    from lns_amd import _lib, dropin, engine, metrics
    header = open(os.path.join(ROOT, "include", "lns.h")).read()
    L = _lib.lib()
    for sym in NEW:
        assert "int %s(" % sym in header, sym
        assert sym in _lib.SYMBOLS and hasattr(L, sym), sym
        assert getattr(L, sym).argtypes is not None, sym
    assert L.lns_build_has(b"eval_stats") == 1
    assert '"eval_stats"' in header and "#define LNS_FIELD_STATS 12" in header
    assert ctypes.sizeof(_lib.LnsStatsSpec) == 72 and _lib.LNS_FIELD_STATS == 12
    for name in ("rollout_eval_stats", "rollout_latent_eval_stats", "field_stats"):
        assert callable(getattr(engine.Engine, name)), name
    assert callable(metrics.field_stats) and callable(metrics.histogram_edges) and callable(metrics.correlation_time)
    assert metrics.FIELD_STATS == fr.NAMES and len(metrics.FIELD_STATS) == 12
    assert callable(dropin.LatentDynamics.validate_stats)
    assert engine.EvalStats._fields == ("frame", "seq", "frames", "stats", "hist", "stats_steps", "spectra", "spectrum_steps")
    assert engine.EvalStatsChunk._fields == engine.EvalStats._fields + ("z_last",)


@pytest.mark.parametrize("name", list(fr.GOLDEN))
def test_float64_reference_reproduces_the_recorded_reference_values(name):
    gold = np.load(os.path.join(ROOT, "tests", "golden", "field_stats.npz"))
    assert int(gold["seed"]) == fr.GOLDEN_SEED
    yh, y = fr.golden_inputs(name)
    got = fr.stats64(torch.from_numpy(yh), torch.from_numpy(y), exact_constants=True, **fr.golden_norm(name)).numpy()
    assert got.dtype == np.float64 and got.shape == fr.GOLDEN[name]["shape"][:3] + (12,)
    for k in ("cos", "grad_y", "grad_x"):
        want = gold["%s_%s" % (name, k)]
        rel = np.abs(got[..., fr.NAMES.index(k)] - want).max() / np.abs(want).max()
        print("%s %s: %.2e" % (name, k, rel))
        assert rel <= 1e-12, (name, k, rel)
    # the statement on the CPU agrees with float64 to fp32 accuracy on every column
    s32 = fr.emulate32(torch.from_numpy(yh), torch.from_numpy(y), **fr.golden_norm(name)).double().numpy()
    ref = fr.stats64(torch.from_numpy(yh), torch.from_numpy(y), **fr.golden_norm(name)).numpy()
    assert np.abs(s32 - ref).max() <= 2e-6 * np.abs(ref).max(axis=(0, 1, 2)).max()


def _family(name, shape, g):
    x = torch.randn(shape, generator=g)
    q = {"unit": x, "tiny": 1e-12 * x, "huge": 1e12 * x, "offset": 1e3 + 1e-2 * x}[name].float()
    return (q + 0.3 * q.std() * torch.randn(shape, generator=g)).float(), q


@pytest.mark.parametrize("family", ["unit", "tiny", "huge", "offset"])
def test_the_statement_is_admissible_under_the_rule(family):
    """The GPU test holds the kernel to max(2e-7, 3 x own) against float64 in both measures.  The statement's reduction
    order, emulated here on the CPU (strided thread sums, pairwise rest), stays at or below 0.68 of that bound on every
    column with torch's CPU reductions as `own`, over planes 3x5 .. 128x128, so the order alone is admissible.  The worst
    ratio of each family is printed."""
    g = torch.Generator().manual_seed(5)
    worst = 0.0
    for plane in ((3, 5), (17, 16), (23, 29), (61, 121), (128, 128)):
        p, q = _family(family, (2, 2, 3) + plane, g)
        ours, own, want = fr.emulate32(p, q), fr.stats32_torch(p, q), fr.stats64(p, q)
        for k, name in enumerate(fr.NAMES):
            def errs(a):
                d = a[..., k].double() - want[..., k]
                return float(d.abs().max() / want[..., k].abs().max()), float(d.norm() / want[..., k].norm())
            ratio = max(a / max(2e-7, 3.0 * b) for a, b in zip(errs(ours), errs(own)))
            worst = max(worst, ratio)
            assert ratio <= 0.68, (family, plane, name, ratio)
    print("%s: statement on the CPU / bound = %.3f" % (family, worst))

def test_bin_rule_on_edge_values():
    f = np.float32
    lo, hi, nbins = f(-0.25), f(1.5), 7
    below, above = np.nextafter(lo, f(-np.inf)), np.nextafter(lo, f(np.inf))
    hbelow, habove = np.nextafter(hi, f(-np.inf)), np.nextafter(hi, f(np.inf))
    v = np.array([lo, hi, below, above, hbelow, habove, np.nan, np.inf, -np.inf, 0.0, -0.0, 1e30, -1e30], f)
    got = fr.bin_rule(v, lo, hi, nbins)
    assert list(got) == [1, nbins + 1, 0, 1, nbins, nbins + 1, -1, nbins + 1, 0, 2, 2, nbins + 1, 0], list(got)
    # every interior value lands in 1 .. nbins, monotonically, and the bins partition [lo, hi) to within one rounding
    x = np.linspace(lo, hbelow, 20001).astype(f)
    b = fr.bin_rule(x, lo, hi, nbins)
    assert b.min() == 1 and b.max() == nbins and np.all(np.diff(b) >= 0)
    from lns_amd import metrics
    edges = metrics.histogram_edges(nbins, float(lo), float(hi)).numpy()
    assert edges.shape == (nbins + 1,) and edges[0] == lo and edges[-1] == hi
    ideal = 1 + np.minimum(nbins - 1, np.floor((x.astype(np.float64) - lo) / (hi - lo) * nbins)).astype(np.int64)
    off = b != ideal
    assert off.mean() < 1e-3 and np.all(np.abs(b - ideal) <= 1)
    near = np.abs(x[off].astype(np.float64)[:, None] - edges[None]).min(1)
    assert off.sum() == 0 or near.max() <= 4e-7 * (hi - lo)
    # nbins = 1 and 256; the product can round up to nbins just below hi: the min keeps it inside
    for n in (1, 256):
        b = fr.bin_rule(np.array([lo, hbelow, hi], f), lo, hi, n)
        assert list(b) == [1, n, n + 1]
    assert metrics.histogram_edges(2, [0.0, 1.0], [1.0, 3.0]).tolist() == [[0.0, 0.5, 1.0], [1.0, 2.0, 3.0]]


def test_correlation_time():
    from lns_amd import metrics
    nan = float("nan")
    corr = torch.tensor([[[0.99, 0.95], [0.85, 0.79], [0.70, 0.90], [0.90, 0.10]],
                         [[0.80, 0.10], [0.81, 0.99], [nan, 0.99], [0.82, 0.99]]])             # [2, 4, 2]
    steps = (0, 8, 16, 24)
    assert metrics.correlation_time(corr, steps).tolist() == [[16, 8], [-1, 0]]
    assert metrics.correlation_time(corr, steps, threshold=0.9).tolist() == [[8, 8], [0, 0]]
    assert metrics.correlation_time(corr, steps, threshold=0.05).tolist() == [[-1, -1], [-1, -1]]
    assert metrics.correlation_time(corr, steps).dtype == torch.int64
    with pytest.raises(Exception, match="n steps"):
        metrics.correlation_time(corr, (0, 8))


# ---- refusals (host only) ---------------------------------------------------------------------------------------------
_P = ctypes.c_void_p(0x1000)
_T = 5


def _ints(*v):
    return (ctypes.c_int * len(v))(*v)


def _engines():
    import copy
    from lns_amd import _lib, config, engine
    mini = config.preset("ns2d_mini")
    big = copy.deepcopy(mini)
    big.Ly = big.Lx = 144                                              # above the spectrum kernel's plane limit
    wide = copy.deepcopy(mini)
    wide.in_channels = 9                                               # above the histograms' channel limit
    mk = lambda a, **kw: engine.Engine(engine.make_config(a, ae_prefix="vq_ae.", prop_prefix="propagator.", **kw))
    engines = {"full": mk(mini), "big": mk(big), "wide": mk(wide), "max4": mk(mini),
               "noprop": mk(mini, prop_kind=_lib.LNS_PROP_NONE)}
    engines["max4"].set_option("eval_max_steps", 4)
    return engines


def _hspec(nbins=16, lo=-1.0, hi=1.0, size=None, edges=None):
    from lns_amd import _lib
    hs = _lib.LnsStatsSpec()
    hs.size = ctypes.sizeof(_lib.LnsStatsSpec) if size is None else size
    hs.nbins = nbins
    for ch in range(8):
        hs.lo[ch], hs.hi[ch] = lo, hi
    for ch, (a, b) in (edges or {}).items():
        hs.lo[ch], hs.hi[ch] = a, b
    return hs


def _call(L, engines, entry, kw):
    from lns_amd import engine
    a = dict(eng="full", start=_P, y=_P, B=3, T=_T, t0=0, Ttot=_T, spec="ok", frame=_P, seq=_P, k=_ints(0, 3, 4), nk=3,
             frames=_P, sel=_ints(0, 3, 4), ns=3, spectra=_P, st=_ints(1, 2, 4), nst=3, hs=_hspec(), stats=_P, hist=_P)
    a.update(kw)
    e = engines[a["eng"]]
    sp = engine.eval_spec(2, mean=0.37, std=1.9)
    if a["spec"] == "bad":
        sp.size = 8
    assert L.lns_set_option(e._h, b"no such option", 0) != 0           # a known last error: was it replaced?
    mark = L.lns_last_error(e._h)
    head = (e._h, a["start"], None, a["y"], a["B"], a["T"])
    mid = (ctypes.byref(sp), a["frame"], a["seq"], a["k"], a["nk"], a["frames"])
    tail = (_P, 1 << 30, None, a["sel"], a["ns"], a["spectra"], a["st"], a["nst"],
            ctypes.byref(a["hs"]) if a["hs"] is not None else None, a["stats"], a["hist"])
    if entry == "lns_rollout_eval_stats":
        rc = L.lns_rollout_eval_stats(*head, *mid, *tail)
    else:
        rc = L.lns_rollout_latent_eval_stats(*head, a["t0"], a["Ttot"], *mid, None, *tail)
    msg = L.lns_last_error(e._h)
    return rc, (None if msg == mark else msg.decode())


_PASSED = (-3, "lns_finalize_weights must be called first")           # every refusal passed: no weights on this machine
_BATCH = (-1, "batch 1073741824 exceeds the maximum of 65535 trajectories per call")
_PLANE = (-1, "energy spectrum: a 144 x 144 plane is not supported (H, W <= 192 and H * W <= 18432)")
_EDGES = (-1, "hspec: the edges of every channel must be finite with hi > lo")
_STEPS = "stats_steps must be ascending steps in [0, 5): entry %d is %d"
_CASES = {
    "valid": (dict(), _PASSED),
    "every_step": (dict(st=_ints(0, 1, 2, 3, 4), nst=5), _PASSED),
    "no_spectra": (dict(sel=None, ns=0, spectra=None), _PASSED),
    "no_histograms": (dict(hs=None, hist=None), _PASSED),
    "description_without_destination": (dict(hist=None), _PASSED),
    "no_kept_frames": (dict(k=None, nk=0, frames=None), _PASSED),
    "big_plane_without_spectra": (dict(eng="big", sel=None, ns=0, spectra=None), _PASSED),
    "wide_without_histograms": (dict(eng="wide", hs=None, hist=None), _PASSED),
    "bad_edge_above_in_channels": (dict(hs=_hspec(edges={3: (1.0, 1.0), 7: (float("nan"), 0.0)})), _PASSED),
    "stats_null": (dict(stats=None), (-1, "stats_out is null")),
    "n_stats_0": (dict(nst=0), (-1, "n_stats must be at least 1")),
    "n_stats_negative": (dict(nst=-1), (-1, "n_stats must be at least 1")),
    "steps_null": (dict(st=None), (-1, "stats_steps is null")),
    "steps_minus_1": (dict(st=_ints(-1, 3, 4)), (-1, _STEPS % (0, -1))),
    "steps_T": (dict(st=_ints(0, 3, 5)), (-1, _STEPS % (2, 5))),
    "steps_unsorted": (dict(st=_ints(0, 4, 3)), (-1, _STEPS % (2, 3))),
    "steps_duplicate": (dict(st=_ints(0, 3, 3)), (-1, _STEPS % (2, 3))),
    "hist_without_hspec": (dict(hs=None), (-1, "hist_out needs a histogram description (hspec is null)")),
    "hspec_size": (dict(hs=_hspec(size=8)), (-1, "hspec: the size field is not sizeof(lns_stats_spec)")),
    "nbins_0": (dict(hs=_hspec(nbins=0)), (-1, "hspec: nbins must be in 1 .. 256")),
    "nbins_257": (dict(hs=_hspec(nbins=257)), (-1, "hspec: nbins must be in 1 .. 256")),
    "nbins_1": (dict(hs=_hspec(nbins=1)), _PASSED),
    "nbins_256": (dict(hs=_hspec(nbins=256)), _PASSED),
    "edge_nan": (dict(hs=_hspec(edges={1: (float("nan"), 1.0)})), _EDGES),
    "edge_inf": (dict(hs=_hspec(edges={0: (0.0, float("inf"))})), _EDGES),
    "edge_equal": (dict(hs=_hspec(edges={1: (0.5, 0.5)})), _EDGES),
    "edge_reversed": (dict(hs=_hspec(lo=1.0, hi=-1.0)), _EDGES),
    "wide_with_histograms": (dict(eng="wide"), (-1, "histograms need in_channels <= 8")),
    # the existing refusals keep their code, message and place ...
    "start_null": (dict(start=None), (-1, None)),
    "y_null": (dict(y=None), (-1, "y_true is null")),
    "spec_bad": (dict(spec="bad"), (-1, "spec is null or its size field is not sizeof(lns_eval_spec)")),
    "keep_unsorted": (dict(k=_ints(0, 4, 3)), (-1, "keep_steps must be ascending steps in [0, 5): entry 2 is 3")),
    "spectra_null": (dict(spectra=None), (-1, "spectra_out is null")),
    "n_spec_negative": (dict(ns=-1), (-1, "n_spec must be at least 1")),
    "spectrum_steps_unsorted": (dict(sel=_ints(0, 4, 3)), (-1, "spectrum_steps must be ascending steps in [0, 5): entry 2 is 3")),
    "plane_unsupported": (dict(eng="big"), _PLANE),
    "B_huge": (dict(B=1 << 30), _BATCH),
    "past_eval_max_steps": (dict(eng="max4"), (-1, "5 steps exceed the option eval_max_steps = 4 (it sizes the evaluation workspace)")),
    "no_propagator": (dict(eng="noprop"), (-3, "rollout needs autoencoder and propagator")),
    # ... and which of two failing checks answers: lns_rollout_eval's, then the spectrum selection's, then the new ones in the
    # written order, then the batch check and the rest
    "stats_null+keep_unsorted": (dict(stats=None, k=_ints(0, 4, 3)), (-1, "keep_steps must be ascending steps in [0, 5): entry 2 is 3")),
    "stats_null+spectra_null": (dict(stats=None, spectra=None), (-1, "spectra_out is null")),
    "stats_null+plane_unsupported": (dict(stats=None, eng="big"), _PLANE),
    "stats_null+n_stats_0": (dict(stats=None, nst=0), (-1, "stats_out is null")),
    "n_stats_0+steps_null": (dict(nst=0, st=None), (-1, "n_stats must be at least 1")),
    "steps_unsorted+hist_without_hspec": (dict(st=_ints(0, 4, 3), hs=None), (-1, _STEPS % (2, 3))),
    "hspec_size+nbins_0": (dict(hs=_hspec(size=8, nbins=0)), (-1, "hspec: the size field is not sizeof(lns_stats_spec)")),
    "nbins_0+edge_equal": (dict(hs=_hspec(nbins=0, edges={0: (0.5, 0.5)})), (-1, "hspec: nbins must be in 1 .. 256")),
    "edge_equal+wide": (dict(eng="wide", hs=_hspec(edges={0: (0.5, 0.5)})), _EDGES),
    "stats_null+B_huge": (dict(stats=None, B=1 << 30), (-1, "stats_out is null")),
    "nbins_257+B_huge": (dict(hs=_hspec(nbins=257), B=1 << 30), (-1, "hspec: nbins must be in 1 .. 256")),
    "steps_T+past_eval_max_steps": (dict(st=_ints(0, 3, 5), eng="max4"), (-1, _STEPS % (2, 5))),
    "n_stats_0+no_propagator": (dict(nst=0, eng="noprop"), (-1, "n_stats must be at least 1")),
}


@pytest.mark.parametrize("entry", ["lns_rollout_eval_stats", "lns_rollout_latent_eval_stats"])
def test_refusal_matrix_of_the_stats_calls(entry):
    from lns_amd import _lib
    L = _lib.lib()
    engines = _engines()
    for name, (kw, (want_rc, want_msg)) in _CASES.items():
        rc, msg = _call(L, engines, entry, kw)
        if name == "start_null":
            want_msg = "x is null" if entry == "lns_rollout_eval_stats" else "z_in is null"
        assert rc == want_rc, (entry, name, rc, msg)
        assert msg == want_msg, (entry, name, msg)
    # the chunked form: the selection is relative to the chunk (T), not to T_total
    rc, msg = _call(L, engines, "lns_rollout_latent_eval_stats", dict(T=2, t0=3, k=_ints(0), nk=1, sel=_ints(1), ns=1, st=_ints(0, 1), nst=2))
    assert (rc, msg) == _PASSED
    rc, msg = _call(L, engines, "lns_rollout_latent_eval_stats", dict(T=2, t0=3, k=_ints(0), nk=1, sel=_ints(1), ns=1, st=_ints(0, 3), nst=2))
    assert (rc, msg) == (-1, "stats_steps must be ascending steps in [0, 2): entry 1 is 3")


def test_python_argument_handling_needs_no_device():
    from lns_amd import engine
    from lns_amd._lib import LnsError
    hs = engine.stats_spec(3, (64, -1.0, [1.0, 2.0, 3.0]))
    assert hs.nbins == 64 and list(hs.lo)[:3] == [-1.0] * 3 and list(hs.hi)[:3] == [1.0, 2.0, 3.0]
    assert engine.stats_spec(3, None) is None
    hs = engine.stats_spec(2, (8, np.float32(-0.5), torch.tensor(2.0)))  # numpy scalars and 0-d tensors are scalar edges
    assert list(hs.lo)[:2] == [-0.5] * 2 and list(hs.hi)[:2] == [2.0] * 2
    hs = engine.stats_spec(2, (8, np.array([0.0, 1.0], np.float32), torch.tensor([2.0, 3.0])))
    assert list(hs.lo)[:2] == [0.0, 1.0] and list(hs.hi)[:2] == [2.0, 3.0]
    with pytest.raises(LnsError, match="one value per channel"):
        engine.stats_spec(3, (64, [0.0, 0.0], 1.0))
    for bad in (None, "0", ["a", "b", "c"]):
        with pytest.raises(LnsError, match="hist: lo must be a number or one value per channel"):
            engine.stats_spec(3, (64, bad, 1.0))


def test_kernels_use_no_scratch_and_spill_nothing():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    from lns_amd import _lib
    res = {k: v for k, v in kernel_resources.resources(_lib.LIB_PATH).items() if "field_stats" in k}
    assert sorted(n.split("field_stats_")[1].split("_kernel")[0] for n in res) == ["group", "stored"], sorted(res)
    for name, r in res.items():
        print(name, r)
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
        assert r["lds"] <= 4096, (name, r)                              # reduction slots and 2 x 258 counts
        assert r["vgpr"] + r["agpr"] <= 128, (name, r)                  # 256 threads: at least four blocks per CU fit the register file

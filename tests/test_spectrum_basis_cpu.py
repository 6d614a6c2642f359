"""CPU: the host side of the energy spectra with a basis per axis (include/lns.h "energy spectra", "a basis per axis"):
exports and bindings, the half-unit bin count against brute force, the float64 reference's own sanity (Parseval, the
single-mode and ramp facts that motivate the DCT), the admissibility of the GPU test's tolerance for the new bases, the
refusals of the op, the bins query and the option (host only), the Python argument handling, the stand-alone check of the
header under sanitizers, and the resources of the built kernels."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import spectrum_basis_reference as br
import spectrum_reference as sr
import test_eval_spectrum_cpu as tsc
from helpers import ROOT

CSRC = tsc.CSRC
NEW = ("lns_spectrum_bins_basis", "lns_op_energy_spectrum_basis")
KNOWN = {(24, 48): (28, 54, 54, 53), (61, 121): (68, 135, 135, 135), (96, 192): (108, 215, 215, 214),
         (128, 128): (92, 181, 181, 181)}


def test_symbols_are_declared_exported_and_bound():
    from lns_amd import _lib, dropin, engine, metrics
    import inspect
    header = open(os.path.join(ROOT, "include", "lns.h")).read()
    L = _lib.lib()
    for sym in NEW:
        assert "int %s(" % sym in header, sym
        assert sym in _lib.SYMBOLS and hasattr(L, sym), sym
        assert getattr(L, sym).argtypes is not None, sym
    assert L.lns_build_has(b"spectrum_basis") == 1
    for text in ('"spectrum_basis"', "#define LNS_SPECTRUM_DFT 0", "#define LNS_SPECTRUM_DCT 1"):
        assert text in header, text
    assert (_lib.LNS_SPECTRUM_DFT, _lib.LNS_SPECTRUM_DCT) == (0, 1) == (br.DFT, br.DCT)
    assert callable(metrics.spectrum_wavenumbers) and callable(metrics.spectrum_basis)
    for fn in (metrics.energy_spectrum, metrics.spectrum_bins, engine.Engine.energy_spectrum, engine.Engine.spectrum_bins,
               engine.Engine.rollout_eval_spectrum, engine.Engine.rollout_latent_eval_spectrum):
        assert inspect.signature(fn).parameters["basis"].default == "dft", fn
    for fn in (engine.Engine.rollout_eval_stats, engine.Engine.rollout_latent_eval_stats, engine.Engine.rollout_eval_maps,
               engine.Engine.rollout_latent_eval_maps, dropin.LatentDynamics.validate_spectrum,
               dropin.LatentDynamics.validate_stats, dropin.LatentDynamics.validate_maps):
        assert inspect.signature(fn).parameters["spectrum_basis"].default == "dft", fn


def test_bins_match_the_brute_force_map():
    from lns_amd import _lib, metrics
    L = _lib.lib()
    planes = [(H, W) for H in range(1, 41) for W in range(1, 41)] + list(KNOWN) + [(192, 96), (121, 61), (1, 192), (192, 1)]
    for H, W in planes:
        assert sr.supported(H, W)
        for by, bx in br.BASES:
            S = L.lns_spectrum_bins_basis(H, W, by, bx)
            assert S == br.bins(H, W, by, bx), (H, W, by, bx)
            if max(H, W) <= 40 or (H, W) in KNOWN:                      # the largest shell any stored mode falls into
                assert S == br.bins_brute(H, W, by, bx), (H, W, by, bx)
            assert 1 <= S <= 256
        assert L.lns_spectrum_bins_basis(H, W, 0, 0) == L.lns_spectrum_bins(H, W)
    for (H, W), want in KNOWN.items():
        assert tuple(L.lns_spectrum_bins_basis(H, W, by, bx) for by, bx in br.BASES) == want
        assert metrics.spectrum_bins(H, W, ("dct", "dft")) == want[1] and metrics.spectrum_bins(H, W, "dct") == want[3]
        assert metrics.spectrum_bins(H, W) == metrics.spectrum_bins(H, W, "dft") == want[0]
    top = max(br.bins(H, W, by, bx) for H in range(1, 193) for W in range(1, 193) if sr.supported(H, W) for by, bx in br.NEW)
    assert top == 215                                                     # one thread per bin still holds
    k = metrics.spectrum_wavenumbers(24, 48, ("dct", "dft"))
    assert k.shape == (54,) and float(k[1]) == 0.5 and float(k[-1]) == 26.5
    k = metrics.spectrum_wavenumbers(24, 48)
    assert k.shape == (28,) and float(k[1]) == 1.0


def test_float64_reference_sanity():
    # dense matrices against numpy.fft for dft / dft
    for H, W in ((1, 7), (3, 5), (24, 40), (29, 57), (32, 32)):
        for name, y_hat, y, norm in sr.cases(H, W):
            a, b = br.spectra64(y_hat, y, (br.DFT, br.DFT), **norm), sr.spectra64(y_hat, y, **norm)
            assert np.abs(a - b).max() <= 1e-11 * np.abs(b).max(), name
    # Parseval for all four bases, odd and even sizes
    for H, W in ((1, 7), (2, 2), (3, 5), (24, 40), (29, 57), (33, 33)):
        for name, y_hat, y, norm in br.cases(H, W):
            fields = sr._fields(y_hat, y, norm, np.float32)
            ms = np.stack([(u.astype(np.float64) ** 2).mean((-2, -1)) for u in fields], -1)
            for basis in br.BASES:
                e = br.spectra64(y_hat, y, basis, **norm)
                assert e.shape == (sr.B, sr.T, sr.C, 3, br.bins(H, W, *basis))
                assert np.abs(e.sum(-1) - ms).max() <= 1e-12 * ms.max(), (name, basis)
                assert np.array_equal(br.spectra64(y_hat, None, basis, **norm)[..., 0, :], e[..., 0, :])
    # a constant field lies in bin 0 under every basis
    const = np.full((1, 1, 1, 24, 40), 1.75)
    for basis in br.BASES:
        e = br.spectra64(const, None, basis, denorm_dtype=np.float64)[0, 0, 0, 0]
        assert abs(e[0] - 1.75 ** 2) <= 1e-12 and np.abs(e[1:]).max() <= 1e-12


def test_wall_mode_and_ramp_facts():
    """What the DCT is for: a wall mode is one bin under (dct, dft) and smeared under (dft, dft); a ramp across the walls
    leaves 6.8e-3 of its energy at 20 cycles and above under the DFT and 4.0e-7 with a DCT along y."""
    mode = br.wall_mode(24, 40, 3, 2)[None, None, None]
    e = br.spectra64(mode, None, (br.DCT, br.DFT), denorm_dtype=np.float64)[0, 0, 0, 0]
    assert abs(e[5] - 0.25) <= 1e-12 and np.abs(np.delete(e, 5)).max() <= 1e-12          # 3^2 + (2 * 2)^2 = 5^2 half cycles
    e = br.spectra64(mode, None, (br.DFT, br.DFT), denorm_dtype=np.float64)[0, 0, 0, 0]
    assert abs(e.sum() - 0.25) <= 1e-12 and abs(e.max() / e.sum() - 0.53) <= 0.005
    u = br.ramp(96, 192)[None, None, None]
    e = br.spectra64(u, None, (br.DFT, br.DFT), denorm_dtype=np.float64)[0, 0, 0, 0]
    tail_dft = e[20:].sum() / e.sum()
    e = br.spectra64(u, None, (br.DCT, br.DFT), denorm_dtype=np.float64)[0, 0, 0, 0]
    tail_dct = e[40:].sum() / e.sum()                                   # bin s lies at s / 2 cycles
    print("ramp 96x192: energy at >= 20 cycles, dft %.3e, dct along y %.3e" % (tail_dft, tail_dct))
    assert abs(tail_dft / 6.8e-3 - 1.0) <= 0.01 and abs(tail_dct / 4.0e-7 - 1.0) <= 0.02


@pytest.mark.parametrize("plane", [(1, 7), (2, 2), (3, 5), (16, 16), (33, 33), (24, 40), (24, 48), (61, 121)], ids=lambda p: "%dx%d" % p)
def test_tolerance_is_admissible(plane):
    """The project's 3 x own rule for the new bases: the float32 numpy statement of the algorithm stays within ONE THIRD of the
    GPU test's bound against the float64 reference, on the GPU test's inputs (spectrum_basis_reference.cases).  Measured worst
    ratio to the bound, (dct,dft) / (dft,dct) / (dct,dct): 3x5 0.037 / 0.026 / 0.030, 24x48 0.055 / 0.024 / 0.033,
    61x121 0.077 / 0.055 / 0.050; 0.077 at most over the planes of this test."""
    H, W = plane
    for basis in br.NEW:
        worst = 0.0
        for name, y_hat, y, norm in br.cases(H, W):
            worst = max(worst, br.worst_ratio(br.spectra32(y_hat, y, basis, **norm), br.spectra64(y_hat, y, basis, **norm)))
        print("%dx%d [%s]: float32 statement / bound = %.4f" % (H, W, br.NAMES[basis], worst))
        assert worst <= 1.0 / 3.0, (basis, worst)
    # the restatement is the DFT one when both axes are DFT
    name, y_hat, y, norm = sr.cases(H, W)[1]
    assert np.array_equal(br.spectra32(y_hat, y, (br.DFT, br.DFT), **norm), sr.spectra32(y_hat, y, **norm))


# ---- refusals (host only: this machine has no device, so a check that came after the first HIP call would answer otherwise) ----
def test_refusals_of_the_op_and_the_bins_query():
    from lns_amd import _lib, engine
    L = _lib.lib()
    for H, W, by, bx in ((129, 144, 1, 1), (1, 193, 1, 0), (0, 4, 0, 1), (4, -1, 1, 1), (32, 32, 2, 0), (32, 32, 0, 2), (32, 32, -1, 1),
                         (32, 32, 1, 3)):
        assert L.lns_spectrum_bins_basis(H, W, by, bx) == _lib.LNS_EINVAL, (H, W, by, bx)
    P = ctypes.c_void_p(0x1000)
    spec = engine.eval_spec(2, mean=0.37, std=1.9)
    bad = engine.eval_spec(2, mean=0.37, std=1.9)
    bad.size = 8
    ok = dict(yhat=P, y=P, B=2, T=2, C=2, H=24, W=40, spec=spec, out=P, by=1, bx=1)
    plane = "energy_spectrum: the plane needs 1 <= H, W <= 192 and H * W <= 18432"
    basis = "energy_spectrum: basis_y, basis_x: LNS_SPECTRUM_DFT (0) or LNS_SPECTRUM_DCT (1)"
    cases = {
        "yhat_null": (dict(yhat=None), "yhat / out is null"),
        "out_null": (dict(out=None), "yhat / out is null"),
        "B_0": (dict(B=0), "B, T, C >= 1 and B * T * C < 2^31"),
        "plane": (dict(H=144, W=144), plane),
        "basis_y_2": (dict(by=2), basis),
        "basis_x_minus_1": (dict(bx=-1), basis),
        "basis_x_3": (dict(by=0, bx=3), basis),
        # which of two failing checks answers: the shape, then the plane, then the basis
        "plane+basis": (dict(H=144, W=144, by=2), plane),
        "B_0+basis": (dict(B=0, bx=2), "B, T, C >= 1 and B * T * C < 2^31"),
    }
    for name, (kw, want) in cases.items():
        a = dict(ok)
        a.update(kw)
        rc = L.lns_op_energy_spectrum_basis(a["yhat"], a["y"], a["B"], a["T"], a["C"], a["H"], a["W"], ctypes.byref(a["spec"]),
                                            a["out"], None, a["by"], a["bx"])
        msg = L.lns_create_error().decode()
        assert rc == _lib.LNS_EINVAL and want in msg, (name, rc, msg)
    rc = L.lns_op_energy_spectrum_basis(P, P, 2, 2, 2, 24, 40, ctypes.byref(bad), P, None, 1, 1)
    assert rc == _lib.LNS_EINVAL


def test_the_option_is_checked_on_the_host_and_changes_no_refusal():
    from lns_amd import _lib
    L = _lib.lib()
    engines = tsc._engines()
    e = engines["full"]
    for v in (-1, 4, 7, 1 << 20):
        assert L.lns_set_option(e._h, b"spectrum_basis", v) == _lib.LNS_EINVAL, v
        assert "spectrum_basis" in L.lns_last_error(e._h).decode()
    for v in (1, 2, 3, 0):
        assert L.lns_set_option(e._h, b"spectrum_basis", v) == 0, v
    with pytest.raises(_lib.LnsError, match="spectrum_basis"):
        e.set_option("spectrum_basis", 4)
    # with a DCT basis selected the streaming entry points refuse what they refused, with the same code and message
    for code in (1, 3):
        for eng in engines.values():
            assert L.lns_set_option(eng._h, b"spectrum_basis", code) == 0
        for entry in ("lns_rollout_eval_spectrum", "lns_rollout_latent_eval_spectrum"):
            for name, (kw, (want_rc, want_msg)) in tsc._CASES.items():
                rc, msg = tsc._call(L, engines, entry, kw)
                if name == "start_null":
                    want_msg = "x is null" if entry == "lns_rollout_eval_spectrum" else "z_in is null"
                assert (rc, msg) == (want_rc, want_msg), (code, entry, name, rc, msg)


def test_python_argument_handling_needs_no_device():
    import torch
    from lns_amd import config, engine, metrics
    from lns_amd._lib import LnsError
    assert metrics.spectrum_basis("dft") == (0, 0) and metrics.spectrum_basis("dct") == (1, 1)
    assert metrics.spectrum_basis(("dct", "dft")) == (1, 0) and metrics.spectrum_basis(["dft", "dct"]) == (0, 1)
    for bad in ("dst", "DCT", 1, None, ("dct",), ("dct", "dft", "dft"), ("dct", 0), "auto"):
        with pytest.raises(LnsError, match="basis"):
            metrics.spectrum_basis(bad)
    x = torch.zeros((1, 1, 1, 4, 4))
    with pytest.raises(LnsError, match="spectrum basis"):
        metrics.energy_spectrum(x, basis="dst")                          # the basis is read before the tensors
    with pytest.raises(LnsError, match="needs a model"):
        metrics.energy_spectrum(x, basis="auto")
    with pytest.raises(LnsError, match="spectrum basis"):
        metrics.spectrum_bins(24, 48, "cosine")
    want = {"ns2d_mini": ("dft", "dft"), "ns2d_64": ("dft", "dft"), "ns2d_128": ("dft", "dft"), "sw_half_periodic": ("dct", "dft"),
            "twophase": ("dct", "dct"), "twophase_cond": ("dct", "dct")}
    for name, names in want.items():
        a = config.preset(name)
        eng = engine.Engine(engine.make_config(a, ae_prefix="vq_ae.", prop_prefix="propagator."))
        assert eng._basis_names("auto") == names, name
        by, bx = metrics.spectrum_basis(names)
        assert eng.spectrum_bins(basis="auto") == br.bins(a.Ly, a.Lx, by, bx), name
        assert eng.spectrum_bins() == sr.bins(a.Ly, a.Lx)
        assert eng.spectrum_bins(24, 48, basis=("dft", "dct")) == 54
        for call in (eng.rollout_eval_spectrum, eng.rollout_latent_eval_spectrum):
            with pytest.raises(LnsError, match="spectrum basis"):
                call(None, None, basis="dst")                            # refused before the tensors are looked at
        for call in (eng.rollout_eval_stats, eng.rollout_latent_eval_stats, eng.rollout_eval_maps, eng.rollout_latent_eval_maps):
            with pytest.raises(LnsError, match="spectrum basis"):
                call(None, None, spectrum_basis=("dct", "dst"))
        # the option is set for the call only
        with eng._spectrum_basis(("dct", "dft")) as got:
            assert got == ("dct", "dft") and eng.options["spectrum_basis"] == 1
        assert eng.options["spectrum_basis"] == 0
        with pytest.raises(RuntimeError, match="inside"):
            with eng._spectrum_basis("dct"):
                assert eng.options["spectrum_basis"] == 3
                raise RuntimeError("inside")
        assert eng.options["spectrum_basis"] == 0


# ---- the host header on its own, under sanitizers ---------------------------------------------------------------------
def test_spectrum_basis_header_stand_alone_under_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "spectrum_basis_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "native", "spectrum_basis_check.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    lines = r.stdout.splitlines()
    assert "planes x bases checked: 16428" in lines
    assert "widest run row (dct y, dft x): 63 of 66" in lines
    for text in ("bins 24x48: 54 / 54 / 53", "bins 61x121: 135 / 135 / 135", "bins 96x192: 215 / 215 / 214",
                 "bins 128x128: 181 / 181 / 181"):
        assert text in lines
    assert "largest S: 215" in lines
    assert "largest LDS request: 155904 bytes" in lines
    assert lines[-1] == "ALL OK"


def test_kernels_with_the_bases_use_no_scratch_and_spill_nothing():
    """The two spectrum kernels now carry the four bases (one launch-uniform switch): still no scratch, no spill, all LDS
    dynamic, two blocks per CU by registers."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    from lns_amd import _lib
    assert _lib.lib().lns_build_has(b"spectrum_basis") == 1
    res = {k: v for k, v in kernel_resources.resources(_lib.LIB_PATH).items() if "spectrum" in k}
    assert len(res) == 2, sorted(res)
    for name, r in res.items():
        print(name, r)
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
        assert r["lds"] == 0 and r["vgpr"] + r["agpr"] <= 256, (name, r)

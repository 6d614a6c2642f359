"""CPU: the composition of two adjacent linear convolutions (csrc/lns_fold.h; DESIGN.md "Folded linear pairs").

The routine is plain host code, so it is checked in a stand-alone program of its own (tests/native/fold_check.cpp) built
with the host compiler under AddressSanitizer and UBSan and run directly: fold_conv_1x1 against a long double loop nest,
element for element, on (k, Cin, Cmid, Cout) = (3, 5, 7, 3), (1, 16, 16, 128), (3, 64, 64, 64) with a bias on A only, on B
only, on both and on neither; fold_pays on the real sites and on shapes where it must say no.

The rest needs no GPU either: the option exists, refuses other values and is documented.  (That the composed packs add
nothing to the parameter table is tests/test_abi_cpu.py::test_param_table_matches_reference_state_dict.)"""
import os
import shutil
import subprocess

import pytest

from helpers import ROOT

CSRC = os.path.join(ROOT, "lns-latent-neural-pde-solver_amd", "csrc")
SHAPES = ("k=3 5->7->3", "k=1 16->16->128", "k=3 64->64->64")


def test_fold_routine_matches_long_double_under_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "fold_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "native", "fold_check.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    lines = r.stdout.splitlines()
    for s in SHAPES:
        for ba in (0, 1):
            for bb in (0, 1):
                assert "fold %s bias_a=%d bias_b=%d: ok" % (s, ba, bb) in lines
    assert "fold_pays decoder tail 3x3 -> 1x1: 1 (expected 1)" in lines
    assert "fold_pays post_quant_conv -> decoder.model.0: 1 (expected 1)" in lines
    assert sum(1 for ln in lines if ln.startswith("fold_pays") and ln.endswith(": 0 (expected 0)")) >= 1
    assert lines[-1] == "ALL OK"


def _engine(preset="ns2d_mini"):
    from lns_amd import config, engine
    a = config.preset(preset)
    return engine.Engine(engine.make_config(a, ae_prefix="vq_ae.", prop_prefix="propagator."))


def test_fold_linear_option_takes_0_and_1_only():
    from lns_amd._lib import LnsError
    e = _engine()
    e.set_option("fold_linear", 0)
    e.set_option("fold_linear", 1)
    for bad in (2, -1):
        with pytest.raises(LnsError, match="fold_linear"):
            e.set_option("fold_linear", bad)
    assert e.options["fold_linear"] == 1


def test_option_is_documented_next_to_the_other_knobs():
    for path in ("README.md", os.path.join("include", "lns.h")):
        text = open(os.path.join(ROOT, path)).read()
        assert "fold_linear" in text and "LNS_NO_FOLD_LINEAR" in text, path

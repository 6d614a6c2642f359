"""CPU: the dual-phase form of the upsampling 3x3 conv (csrc/conv3_up2d.inc).

What needs no GPU: the kernel's resources in the built gfx950 code object (two blocks per CU: no scratch, no spills, at most
256 registers per wave, at most 80 KB of LDS at the largest shape the per-layer rule admits), the rule itself (a stand-alone
program, tests/native/up2d_fit_check.cpp, linked against the built library and calling host functions only), and the
`up2_dual` option."""
import os
import shutil
import subprocess
import sys

import pytest

from helpers import ROOT

CSRC = os.path.join(ROOT, "lns-latent-neural-pde-solver_amd", "csrc")
LDS_BUDGET = 80 * 1024


@pytest.fixture(scope="module")
def fit_lines(tmp_path_factory):
    from lns_amd import _lib
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    libdir = os.path.dirname(os.path.abspath(_lib.LIB_PATH))
    exe = str(tmp_path_factory.mktemp("up2d") / "up2d_fit_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), "-I", CSRC,
                           os.path.join(ROOT, "tests", "native", "up2d_fit_check.cpp"), "-o", exe,
                           "-L", libdir, "-l:" + os.path.basename(_lib.LIB_PATH), "-Wl,-rpath," + libdir,
                           "-Wl,-rpath," + os.path.join(rocm, "lib")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    lines = r.stdout.splitlines()
    assert lines[-1] == "ALL DONE"
    return lines


def _field(lines, prefix, key):
    ln = [x for x in lines if x.startswith(prefix)]
    assert len(ln) == 1, (prefix, lines)
    words = ln[0][len(prefix):].split()
    return int(words[words.index(key) + 1])


def test_kernel_resources_allow_two_blocks_per_cu(fit_lines):
    from lns_amd import _lib
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    res = {k: v for k, v in kernel_resources.resources(_lib.LIB_PATH).items() if "conv3_up2d_kernel" in k}
    assert len(res) == 1, "the dual-phase kernel is compiled into the normal build, once: %s" % sorted(res)
    (name, r), = res.items()
    print(name, r)
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0, r
    assert r["vgpr"] + r["agpr"] <= 256, r
    dyn = _field(fit_lines, "largest:", "lds")
    assert _field(fit_lines, "largest:", "fits") == 1
    assert r["lds"] + dyn <= LDS_BUDGET, (r["lds"], dyn)


def test_fit_rule(fit_lines):
    # the decoder's layers: a 4 x 32 source tile with its halo, eight stages -- about 50 KB
    assert _field(fit_lines, "decoder layer 64->64 at 128^2:", "fits") == 1
    assert 2 * (205 * 32 + 16384) <= _field(fit_lines, "decoder layer 64->64 at 128^2:", "lds") <= 52 * 1024
    assert _field(fit_lines, "patch 256:", "fits") == 1 and _field(fit_lines, "patch 257:", "fits") == 0
    # the LDS bound is what ends the admitted range of channel counts
    assert _field(fit_lines, "largest:", "lds") <= LDS_BUDGET < _field(fit_lines, "past the largest:", "lds")
    assert _field(fit_lines, "past the largest:", "fits") == 0
    refused = [ln for ln in fit_lines if ln.startswith("refuse ")]
    assert len(refused) == 8 and all(ln.endswith(": 0") for ln in refused), refused
    assert _field(fit_lines, "residual, ragged channels:", "fits") == 1


def _engine(preset="ns2d_mini"):
    from lns_amd import config, engine
    a = config.preset(preset)
    return engine.Engine(engine.make_config(a, ae_prefix="vq_ae.", prop_prefix="propagator."))


def test_up2_dual_option_takes_0_and_1_only():
    from lns_amd._lib import LnsError
    e = _engine()
    e.set_option("up2_dual", 0)
    e.set_option("up2_dual", 1)
    for bad in (2, -1):
        with pytest.raises(LnsError, match="up2_dual"):
            e.set_option("up2_dual", bad)
    assert e.options["up2_dual"] == 1


def test_option_is_documented_next_to_the_other_knobs():
    for path in ("README.md", os.path.join("include", "lns.h")):
        text = open(os.path.join(ROOT, path)).read()
        assert "up2_dual" in text and "LNS_UP2_DUAL" in text, path

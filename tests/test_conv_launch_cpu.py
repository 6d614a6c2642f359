"""CPU: the host rules that build a convolution launch (csrc/lns_conv_launch.h), shared by the planner, the op-level entry
points, the training plans and the model builder.  A stand-alone program, tests/native/conv_launch_check.cpp, is linked against
the built library and calls host functions only; every value pinned here is derived by hand from the rule, in the comment
beside it."""
import math
import os
import re
import shutil
import subprocess

import pytest

from helpers import ROOT

CSRC = os.path.join(ROOT, "lns-latent-neural-pde-solver_amd", "csrc")


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    from lns_amd import _lib
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    libdir = os.path.dirname(os.path.abspath(_lib.LIB_PATH))
    exe = str(tmp_path_factory.mktemp("conv_launch") / "conv_launch_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), "-I", CSRC,
                           os.path.join(ROOT, "tests", "native", "conv_launch_check.cpp"), "-o", exe,
                           "-L", libdir, "-l:" + os.path.basename(_lib.LIB_PATH), "-Wl,-rpath," + libdir,
                           "-Wl,-rpath," + os.path.join(rocm, "lib")])
    env = {k: v for k, v in os.environ.items() if not k.startswith("LNS_")}      # the rules' A/B knobs at their defaults
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, env=env)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    out = r.stdout.splitlines()
    assert out[-1] == "ALL DONE"
    return out


def _line(lines, prefix):
    ln = [x for x in lines if x.startswith(prefix)]
    assert len(ln) == 1, (prefix, lines)
    return ln[0][len(prefix):].strip()


def _fields(lines, prefix):
    """'key value key value ...' after the prefix -> {key: number}"""
    w = _line(lines, prefix).split()
    assert len(w) % 2 == 0, w
    return {k: float(v) if re.search(r"[.e]", v) else int(v) for k, v in zip(w[::2], w[1::2])}


def test_padded_sizes(lines):
    # 3x3: stages of 8 input channels, 1x1: of 32; 32 / 64 output channels, then multiples of 128
    assert _fields(lines, "padded k3 3->4:") == dict(kc_log2=3, Cin_pad=8, Cout_pad=32)
    assert _fields(lines, "padded k1 40->100:") == dict(kc_log2=5, Cin_pad=64, Cout_pad=128)
    for cout, want in ((33, 64), (64, 64), (65, 128), (129, 256)):
        assert _fields(lines, "padded cout %d:" % cout) == dict(Cout_pad=want)


def test_weight_scale(lines):
    # the largest power of two S with S * max|w| <= 16000: 2^13 = 8192 <= 16000 < 2^14
    assert float(_line(lines, "scale max 1:")) == 8192.0
    assert float(_line(lines, "scale max 2:")) == 4096.0
    assert float(_line(lines, "scale max 16000:")) == 1.0
    assert float(_line(lines, "scale max 16001:")) == 0.5
    # 1 / S for the kernels whose slabs hold w * S (f16x2 3x3, split 1x1), 1 for the fp32 kernels
    assert _fields(lines, "unscale:") == dict(f16x2=1.0 / 4096, b1=0.125, fp32=1)


def test_patch_division_constant(lines):
    # ceil(2^32 / PH); PH = 1 needs no division
    assert int(_line(lines, "ph_magic PH 1:")) == 0
    assert int(_line(lines, "ph_magic PH 6:")) == 715827883          # 2^32 / 6 = 715827882.67
    assert int(_line(lines, "ph_magic PH 34:")) == -((-2 ** 32) // 34) == 126322568


def test_arithmetic_maps_rule(lines):
    # variant 11 on a 16 x 16 plane, pad 1: on; map_circ per axis from the padding mode, map_pad the low pads,
    # map_ext = size + both pads = 18
    for name, cy, cx in (("zeros zeros", 0, 0), ("circular zeros", 1, 0), ("zeros circular", 0, 1), ("circular circular", 1, 1)):
        assert _line(lines, "arith %s:" % name) == "on 1 circ %d %d pad 1 1 ext 18 18" % (cy, cx)
    # pads up to the plane (one period) are fine, whatever the dilation: 16 + 4 + 4 = 24
    assert _line(lines, "arith pad 4 dilation 4:") == "on 1 circ 1 1 pad 4 4 ext 24 24"
    for name in ("fp32 variant", "resized 2x, not the phase form", "pad 17", "other padding mode"):
        assert _line(lines, "arith %s:" % name) == "on 0 circ 0 0 pad 0 0 ext 0 0"


def test_map_lengths_and_ends(lines):
    t = _fields(lines, "tiling 21x37:")
    assert t["found"] == 1 and t["TN"] == 128
    BW = 1 << t["bw_log2"]
    BH = t["TN"] // BW
    # covered area per tile shape: 16 x 8 tiles 48 * 24 = 1152 < 8 x 16: 40 * 32 < 64 x 2: 64 * 22 < 32 x 4: 64 * 24 < 128 x 1
    assert (BW, BH) == (16, 8)
    assert (t["tiles_x"], t["tiles_y"]) == (math.ceil(37 / BW), math.ceil(21 / BH)) == (3, 3)
    assert (t["PH"], t["PW"]) == (BH + 2, BW + 2)
    r = _fields(lines, "rowmap:")
    c = _fields(lines, "colmap:")
    assert r["len"] == (t["tiles_y"] - 1) * BH + t["PH"] == 26 and c["len"] == (t["tiles_x"] - 1) * BW + t["PW"] == 50
    # rows circular: padded row 0 is source row 20, row 22 wraps to 0; past 21 + 2 padded rows nothing is read
    assert (r["r0"], r["r1"], r["r21"], r["r22"], r["r23"], r["last"]) == (20, 0, 20, 0, -1, -1)
    # columns zeros: the pad columns read nothing
    assert (c["c0"], c["c1"], c["c37"], c["c38"], c["last"]) == (-1, 0, 36, -1, -1)


def test_groupnorm_fold_and_bound(lines):
    # 128 pixels per partial is the kernel's default (0); one ragged tile passes the plane's count; the table is dropped
    assert _fields(lines, "fold exact tiles:") == dict(gn_count=0, gn_tiles=2, gn_groups=32, ss_null=1, part=1, gamma=1, beta=1,
                                                      premul_null=1, eps=1e-6)
    assert _fields(lines, "fold ragged single tile:") == dict(gn_count=105, gn_tiles=1, gn_groups=1, ss_null=1, premul=1)
    # max|gamma| sqrt(channels per group * H * W) + max|beta| = 2 sqrt(8 * 16) + 0.5
    # (fp32: a few 1e-6 at 23.1), handed over as the final bound of the consumer's input: no per-sample maximum is read
    b = _fields(lines, "gn bound:")
    assert abs(b["value"] - (2 * math.sqrt(128) + 0.5)) < 5e-6 and (b["final"], b["amax_null"]) == (1, 1)


def test_geometry_to_conv_args(lines):
    # ConvGeom {variant 11, bw_log2 4, tiles 3 x 5, 2 cout tiles, patch 10 x 18, 21 x 37 out, kc_log2 3, selected 2},
    # B 7, 40 x 21 x 37 in, 100 out, 3x3 stride 1 dilation 2, pads 40 / 128: ceil(2^32 / 10) = 429496730
    assert _fields(lines, "geom:") == dict(kc_log2=2, tiles_x=3, tiles_y=5, cout_tiles=2, bw_log2=4, PH=10, PW=18, B=7,
                                           ph_magic=429496730, ks=3, stride=1, dil=2, Cin_pad=40, Cout_pad=128, vec4=0, Cin=40,
                                           Hin=21, Win=37, Cout=100, Hout=21, Wout=37, x_bs=40 * 21 * 37, y_bs=100 * 21 * 37)
    # 16-byte patch loads of a 1x1: a plane of a multiple of four pixels
    assert int(_line(lines, "vec4 1x1 on 16 pixels:")) == 1 and int(_line(lines, "vec4 1x1 on 777 pixels:")) == 0

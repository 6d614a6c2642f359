"""CPU: the switch table (csrc/lns_knobs.h) and the form rules planner and launcher share (attn_is_f16, fa_sandwich_form).
A stand-alone program, tests/native/knobs_check.cpp, is linked against the built library and calls host functions only, one
child process per environment.  Every default pinned here was copied by hand from the getenv site the table replaced (file and
line of the commit before the table, in the comment beside it); every expected form is derived by hand from that commit's
launch_fa_sandwich_t / launch_attention, as the comment above FORMS says."""
import os
import re
import shutil
import subprocess

import pytest

from helpers import ROOT

CSRC = os.path.join(ROOT, "lns-latent-neural-pde-solver_amd", "csrc")

# name -> default.  Flags print 0 / 1 (`getenv(...) != nullptr`), counts the number (atol / atoi of the value).
DEFAULTS = {
    "LNS_GN_NO_FUSE": 0,                # lns_engine.cpp:291   static const bool off = getenv(..) != nullptr
    "LNS_GN_NO_FOLD": 0,                # lns_engine.cpp:83
    "LNS_GN_FUSE_MIN_HW": 256,          # lns_engine.cpp:84    ... : (no_fold ? 1024 : 256)
    "LNS_GN_NO_RAGGED": 0,              # lns_engine.cpp:93
    "LNS_GN_NO_RAGGED_TILES": 0,        # lns_engine.cpp:97
    "LNS_GN_FOLD_TILES": 2,             # lns_engine.cpp:113   ... : 2
    "LNS_CONV_FP32_MFMA": 0,            # lns_conv_launch.h:76, lns_engine.cpp:440, 719, 1063
    "LNS_CONV1_FP32_MFMA": 0,           # lns_conv_launch.h:81, lns_engine.cpp:720
    "LNS_CONV1_NO_THIN": 0,             # lns_conv_launch.h:87
    "LNS_CONV1_NO_STATIONARY": 0,       # lns_engine.cpp:503
    "LNS_CONV1S_MIN_BLOCKS": 512,       # lns_engine.cpp:505   ... : 512
    "LNS_CONV_USE_128": 0,              # lns_conv_launch.h:71
    "LNS_CONV_MIN_BLOCKS": 128,         # lns_conv_launch.h:138  ... : 128
    "LNS_CONVB32_BELOW": 0,             # lns_conv_launch.h:143  ... : 0
    "LNS_CONVF32_BELOW": 100,           # lns_conv_launch.h:152  ... : 100
    "LNS_CONV_KCL4": 0,                 # lns_kernels.hip:757
    "LNS_CONV_W8_BELOW": 0,             # lns_kernels.hip:2601   ... : 0
    "LNS_CONV3_SPLIT": "f16x2",         # lns_engine.cpp:1268  conv3_f16 = !(set && strcmp(.., "bf16x3") == 0)
    "LNS_NO_FUSE_1X1": 0,               # lns_engine.cpp:429
    "LNS_NO_GELU_PROLOGUE": 0,          # lns_engine.cpp:1063
    "LNS_NO_ARITH_MAPS": 0,             # lns_conv_launch.h:192
    "LNS_NO_UP2_PHASES": 0,             # lns_engine.cpp:1246
    "LNS_UP2_QUAD": 0,                  # lns_engine.cpp:465   no_quad = getenv(QUAD) == nullptr || getenv(RESIDENT) != nullptr
    "LNS_UP2_RESIDENT": 0,              # lns_engine.cpp:465, 546
    "LNS_FA_SANDWICH_FP32": 0,          # lns_kernels.hip:4631, lns_engine.cpp:719, 886
    "LNS_FA_SANDWICH_BF16X3": 0,        # lns_kernels.hip:4640, lns_engine.cpp:720
    "LNS_FA_SANDWICH_3WAVE": 0,         # lns_kernels.hip:4636
    "LNS_FA_PPB": 64,                   # lns_kernels.hip:4643, 4660  ... : 64
    "LNS_FA_FUSED_NO_SMALL": 0,         # lns_engine.cpp:721
    "LNS_FA_NO_FUSE_TO_OUT": 0,         # lns_engine.cpp:761, 898
    "LNS_FA_NO_MERGE": 0,               # lns_engine.cpp:766
    "LNS_FA_NO_REVERSE": 0,             # lns_engine.cpp:862, 880
    "LNS_FA_REDUCER_SCALAR": 0,         # lns_kernels.hip:3750
    "LNS_ATTN_FP32": 0,                 # lns_kernels.hip:3437, lns_engine.cpp:656
    "LNS_WGRAD_TARGET_BLOCKS": 512,     # wgrad_split.inc:36, 47  WG_TARGET_BLOCKS
    "LNS_WGRAD_MAX_SLICES": 128,        # wgrad_split.inc:37, 48  WG_MAX_SLICES
    "LNS_DEBUG_SYNC": 0,                # lns_engine.cpp:1577
    "LNS_TIMING_BY_NAME": 0,            # lns_engine.cpp:1598
    # option defaults: lns_create (lns_engine.cpp:1949-1957) overrode the initialisers of lns_engine.h when the variable was set
    "LNS_DECODE_GROUP": 1,              # lns_engine.h:171  opt_decode_group = 1
    "LNS_DECODE_STREAMS": 3,            # lns_engine.h:172  opt_decode_streams = 3
    "LNS_NO_OVERLAP": 0,                # lns_engine.h:174  opt_overlap = 1; set: 0
    "LNS_PROP_PRIORITY": 0,             # lns_engine.h:175  opt_prop_priority = 0; set: 1
    "LNS_FA_CHUNK_MB": 0,               # lns_engine.h:179  opt_fa_chunk_mb = 0
    "LNS_FA_FUSED": 2,                  # lns_engine.h:182  opt_fa_fused = 2
    "LNS_FA_FUSED_GPB": 0,              # lns_engine.h:184  opt_fa_fused_gpb = 0
    "LNS_NO_FOLD_LINEAR": 0,            # lns_engine.h:187  opt_fold_linear = 1; set: 0
    "LNS_UP2_DUAL": 1,                  # lns_engine.h:190  opt_up2_dual = 1
}
COUNT = 7         # a value no count has as its default


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    from lns_amd import _lib
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    libdir = os.path.dirname(os.path.abspath(_lib.LIB_PATH))
    exe = str(tmp_path_factory.mktemp("knobs") / "knobs_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"),
                           "-I", CSRC, os.path.join(ROOT, "tests", "native", "knobs_check.cpp"), "-o", exe,
                           "-L", libdir, "-l:" + os.path.basename(_lib.LIB_PATH), "-Wl,-rpath," + libdir,
                           "-Wl,-rpath," + os.path.join(rocm, "lib")])
    base = {k: v for k, v in os.environ.items() if not k.startswith("LNS_")}

    def go(mode, **env):
        r = subprocess.run([exe, mode], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, env=dict(base, **env))
        assert r.returncode == 0, r.stdout
        out = r.stdout.splitlines()
        assert out[-1] == "ALL DONE", r.stdout
        return out[:-1]
    return go


def values(run, **env):
    rec = {}
    for ln in run("values", **env):
        name, v = ln.split()
        rec[name] = v if name == "LNS_CONV3_SPLIT" else int(v)
    return rec


@pytest.fixture(scope="module")
def rows(run):
    r = [ln.split("\t") for ln in run("rows")]
    assert all(len(x) == 4 for x in r), r
    return r


def test_defaults(run, rows):
    assert values(run) == DEFAULTS
    assert [r[0] for r in rows] == list(DEFAULTS)                    # a row per switch, none twice
    # the default text of a row is what an unset variable parses
    for name, kind, dflt, _ in rows:
        want = DEFAULTS[name]
        assert dflt == ("off" if want == 0 and "flag" in kind else str(want)), (name, dflt)


def test_isolation(run, rows):
    for name, kind, _, _ in rows:
        if name == "LNS_CONV3_SPLIT":
            assert values(run, **{name: "bf16x3"}) == dict(DEFAULTS, **{name: "bf16x3"})
            assert values(run, **{name: "bf16"}) == DEFAULTS             # any other string: the default
            continue
        setting, got = ("1", 1) if "flag" in kind else (str(COUNT), COUNT)
        want = dict(DEFAULTS, **{name: got})
        if name == "LNS_GN_NO_FOLD":
            want["LNS_GN_FUSE_MIN_HW"] = 1024                            # coupled default (lns_engine.cpp:84)
        assert values(run, **{name: setting}) == want, name
    # a flag is "set or not": the empty string and 0 switch it on as well
    assert values(run, LNS_ATTN_FP32="")["LNS_ATTN_FP32"] == 1 and values(run, LNS_ATTN_FP32="0")["LNS_ATTN_FP32"] == 1
    # the couplings: an explicit LNS_GN_FUSE_MIN_HW wins over LNS_GN_NO_FOLD's default; LNS_UP2_QUAD is inert under LNS_UP2_RESIDENT
    assert values(run, LNS_GN_NO_FOLD="1", LNS_GN_FUSE_MIN_HW="300")["LNS_GN_FUSE_MIN_HW"] == 300
    assert values(run, LNS_UP2_QUAD="1", LNS_UP2_RESIDENT="1") == dict(DEFAULTS, LNS_UP2_RESIDENT=1)
    # weight-gradient slice rule: values below 1 fall back to the default (wgrad_split.inc:43, `return v >= 1 ? v : dflt`)
    assert values(run, LNS_WGRAD_TARGET_BLOCKS="0", LNS_WGRAD_MAX_SLICES="-3") == DEFAULTS


def test_read_once(run):
    before, after = run("once")
    assert before == "LNS_GN_NO_FUSE 0 LNS_FA_PPB 64 LNS_DECODE_GROUP 1"
    # the process switches keep what the first call read; the option default, parsed again, sees the change
    assert after == "LNS_GN_NO_FUSE 0 LNS_FA_PPB 64 LNS_DECODE_GROUP 5"


# launch_fa_sandwich_t<HT, WT> before the table (lns_kernels.hip:4628-4682), HT x WT tiles of 32 x 32, LDS limit 160 KB = 163840:
#   1. f16x2 if WT <= 3, not LNS_FA_SANDWICH_FP32, not LNS_FA_SANDWICH_BF16X3, amax_u given, and its image fits:
#      (2 HB (HB + 8) + 2 WB (WB + 8) + 8 * 32 (WB + 8)) * 2 + 64 bytes, HB = 32 HT, WB = 32 WT; the largest, 64 x 96:
#      (9216 + 19968 + 26624) * 2 + 64 = 111680: fits on all five tilings.
#   2. else bf16x3 if not LNS_FA_SANDWICH_FP32, (NWV == 4 or LNS_FA_SANDWICH_3WAVE) and the NWV-wave image fits, where NWV = 4
#      if the four-wave image (3 HB (HB + 8) + 3 WB (WB + 8) + NWV * 3 * 32 (WB + 8)) * 2 fits, else 3:
#      32x32 46080, 32x64 90624, 64x64 110592, 64x32 66048: four waves.  64x96: (13824 + 29952 + 39936) * 2 = 167424 > 163840,
#      so NWV = 3: (13824 + 29952 + 29952) * 2 = 147456 fits -- under LNS_FA_SANDWICH_3WAVE only.
#   3. else fp32 MFMA if (HB (HB + 1) + WB (WB + 1) + 128 (WB + 1)) * 4 fits: 64x96 103552, the largest: always.
# launch_fa_sandwich (:4684-4692) has these five tilings only: a 96 x 192 plane (3 x 6 tiles) returned hipErrorInvalidValue.
# launch_attention (:3437-3438): f16x2 if amax_in given and not LNS_ATTN_FP32.
PLANES = ("32x32", "32x64", "64x64", "64x96", "64x32")
NO_AMAX = {p: "bf16x3" for p in PLANES}
NO_AMAX["64x96"] = "fp32"
FORMS = {
    "default": ({p: "f16x2" for p in PLANES}, NO_AMAX),
    "LNS_FA_SANDWICH_FP32": ({p: "fp32" for p in PLANES}, {p: "fp32" for p in PLANES}),
    "LNS_FA_SANDWICH_BF16X3": (NO_AMAX, NO_AMAX),
    "LNS_FA_SANDWICH_3WAVE": ({p: "f16x2" for p in PLANES}, dict(NO_AMAX, **{"64x96": "bf16x3_3wave"})),
    "LNS_ATTN_FP32": ({p: "f16x2" for p in PLANES}, NO_AMAX),
}


@pytest.mark.parametrize("arm", list(FORMS))
def test_form_rules(run, arm):
    got = {}
    for ln in run("forms", **({} if arm == "default" else {arm: "1"})):
        m = re.fullmatch(r"(\d+x\d+) amax ([01]): sandwich (\w+) attn_f16 ([01])", ln)
        assert m, ln
        got[m.group(1), int(m.group(2))] = (m.group(3), int(m.group(4)))
    with_amax, without = FORMS[arm]
    want = {}
    for p in PLANES:
        want[p, 1] = (with_amax[p], 0 if arm == "LNS_ATTN_FP32" else 1)
        want[p, 0] = (without[p], 0)
    for amax in (0, 1):
        want["96x192", amax] = ("none", want["32x32", amax][1])
    assert got == want


def test_inventory(rows):
    # getenv( in csrc/: the table's parser, and the reads of diagnostic builds
    allowed = {"lns_engine.cpp": r"LNS_TS_|LNS_SKIP_OPS", "lns_ops.inc": r"LNS_STRESS_"}
    for fn in sorted(os.listdir(CSRC)):
        if fn == "lns_knobs.h" or not fn.endswith((".h", ".hip", ".cpp", ".inc")):
            continue
        for i, ln in enumerate(open(os.path.join(CSRC, fn)), 1):
            if "getenv(" in ln:
                assert fn in allowed and re.search(allowed[fn], ln), "%s:%d: %s" % (fn, i, ln.strip())
    # README's environment table: one line per row, the same default text; every LNS_ name in it is a row
    table = [ln for ln in open(os.path.join(ROOT, "README.md")) if ln.startswith("| `LNS_")]
    doc = {}
    for ln in table:
        cells = [c.strip() for c in ln.strip().strip("|").split("|")]
        assert len(cells) == 3, ln
        doc[cells[0].strip("`")] = cells[1:]
    names = [r[0] for r in rows]
    assert list(doc) == names
    for name, _, dflt, meaning in rows:
        assert doc[name] == [dflt, meaning], name
    assert set(re.findall(r"LNS_[A-Z0-9_]+", "".join(table))) == set(names)

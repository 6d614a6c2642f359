"""CPU: the float64 statements of tests/fa_axis_reference.py against the float32 oracle on every reducer and low-rank-kernel
input set the GPU tests launch (the oracle's own error is what the non-default tolerances are made of), the host rotary table
bit for bit, the two fit predicates, and the argument checks of lns_op_fa_reducer / lns_op_fa_lrk -- they precede the first HIP
call, so they need no device.  (A plan can only be built on finalized weights, which need a device: the plan-time refusal of
a 128-channel FABlock is in tests/test_fa_axis_gpu.py.)"""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

import fa_axis_reference as fr
from helpers import ROOT


def _L():
    from lns_amd import _lib
    return _lib.lib()


# ---- reference against the oracle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", fr.KINDS)
def test_reducer_statement_agrees_with_the_oracle(kind):
    """lns_oracle._pooling_reducer (after the pool) on every set of the kind: within ORACLE_TOL of float64 on the zero-mean
    sets; on the offset sets the measured error, times TOL_FACTOR, is the set's tolerance and must stay a usable one."""
    for s in [s for s in fr.reducer_sets() if s[0] == kind]:
        r = fr.reducer_set(*s)
        print("reducer %-36s oracle rel-L2 per sample, worst %.2e -> tolerance %.2e" % (r["name"], r["oracle_err"].max(), r["tol"]))
        assert np.isfinite(r["ref"]).all() and r["ref"].shape == (r["B"], r["Out"], r["n"])
        if kind in fr.MEASURED_KINDS:
            # (a mean of three standard deviations costs LayerNorm about two bits: the rule may not give more than 2 x KERNEL_TOL)
            assert r["tol"] == fr.TOL_FACTOR * r["oracle_err"].max() and 0.0 < r["tol"] < 2 * fr.KERNEL_TOL, r["name"]
        else:
            assert r["oracle_err"].max() < fr.ORACLE_TOL and r["tol"] == fr.KERNEL_TOL, (r["name"], r["oracle_err"])


def test_reducer_sets_are_what_their_kind_says():
    """The conditioning LayerNorm sees, |mean| / std over the channels of a row after to_in, median over a sample's rows.  A
    per-channel offset of the pooled rows does NOT reach LayerNorm: a random to_in turns it into another zero-mean vector, and
    the `offset` sets sit where the zero-mean sets do (below 0.3).  The `ln_offset` sets carry the offset that to_in maps to a
    common value: LN_SHIFTS standard deviations, 3 at sample 0."""
    for s in fr.reducer_sets():
        r = fr.reducer_set(*s)
        t = r["m"].astype(np.float64) @ r["w"][r["tag"] + ".to_in.weight"].astype(np.float64).T
        with np.errstate(invalid="ignore"):
            ratio = np.nanmedian(np.abs(t.mean(axis=-1)) / t.std(axis=-1), axis=1)          # [B] (the zero row of const_row: nan)
        if r["kind"] == "offset":
            assert np.abs(r["m"].mean(axis=1)).max() > 2.0                       # offsets of up to 3 standard deviations
        if r["kind"] == "ln_offset":
            want = np.abs([fr.LN_SHIFTS[b % 3] for b in range(r["B"])])
            assert np.abs(ratio / want - 1.0).max() < 0.2 and ratio[0] > 2.5, (r["name"], ratio)
            assert np.abs(r["m"]).max() < 20.0, r["name"]                        # a few standard deviations per channel
        else:
            assert ratio.max() < 0.3, (r["name"], ratio)
        if r["kind"] == "const_row":
            want = fr.reducer_beta_row64(r["w"], r["tag"])
            for b, i in enumerate(fr.const_rows(r["B"], r["n"])):
                assert not r["m"][b, i].any() and np.allclose(r["ref"][b, :, i], want, rtol=1e-12, atol=0)


@pytest.mark.parametrize("freq", fr.FREQS)
def test_lrk_statement_agrees_with_the_oracle(freq):
    """lns_oracle._low_rank_kernel per (sample, head).  The oracle takes its positions from numpy's linspace, the statement
    from torch's (as the reference does): they differ by an ulp at some positions, times an angle scale of 64 (std) or 640
    (x10) -- except at n = 33, where the step 1 / 32 is exact.  That is a difference of definitions, not a rounding error, so
    the oracle's own error is measured against the statement on the oracle's positions (1.3e-7 .. 2.3e-7 on every set); against
    the statement on torch's positions it would read up to 8.9e-7 (std) and 8.9e-6 (x10) and hide a kernel that lost 1e-5."""
    for s in [s for s in fr.lrk_sets() if s[0] == freq]:
        r = fr.lrk_set(*s)
        print("lrk %-28s oracle rel-L2 per (sample, head), worst %.2e -> tolerance %.2e" % (r["name"], r["oracle_err"].max(), r["tol"]))
        assert r["ref"].shape == (r["B"], r["heads"], r["n"], r["n"]) and np.isfinite(r["ref"]).all()
        mixed = fr.rel_l2(fr.lrk_oracle(r["qk"], r["heads"], r["DK"], r["invf"]), r["ref"], 2).max()
        assert r["n"] != 33 or mixed == r["oracle_err"].max(), r["name"]              # exact positions: one definition
        # (two float32 orders of a DK-term product sum: a few 1e-7; the rule may not give more than KERNEL_TOL / 2)
        assert r["tol"] == fr.TOL_FACTOR * r["oracle_err"].max() and 0.0 < r["tol"] < fr.KERNEL_TOL / 2, r["name"]
        # no scaling is hidden anywhere: the result carries the product of the two scales
        h = r["heads"] * r["DK"]
        unscaled = np.concatenate([r["qk"][:, :h] / np.float32(fr.Q_SCALE), r["qk"][:, h:] / np.float32(fr.K_SCALE)], axis=1)
        k1 = fr.lrk64(unscaled, r["heads"], r["DK"], r["invf"])
        assert np.allclose(r["ref"], k1 * (fr.Q_SCALE * fr.K_SCALE), rtol=1e-6, atol=0.3 * 1e-6 * np.abs(r["ref"]).max())


def test_chain_statement_agrees_with_the_oracle():
    """The chain's input set (tests/test_fa_axis_gpu.py::test_chain_pool_reducer_to_qk_lrk) through the oracle in the reference's
    order, Linear before the mean: the reducer outputs within ORACLE_TOL; Kx / Ky -- three chained float32 stages, reducer, to_qk
    and the low-rank kernel, each within ORACLE_TOL -- within 3 x ORACLE_TOL of the statement on the oracle's positions, which
    leaves KERNEL_TOL, the GPU test's bound, a margin."""
    c, o = fr.chain_set(), fr.chain_oracle()
    for ax in "xy":
        eu = fr.rel_l2(o["u" + ax], c["ref"]["u" + ax], 1)
        ek = fr.rel_l2(o["k" + ax], c["ref"]["k%s@oracle" % ax], 2)
        print("chain %s: oracle u rel-L2 per sample %.2e, K per (sample, head) %.2e" % (ax, eu.max(), ek.max()))
        assert eu.max() < fr.ORACLE_TOL and ek.max() < 3 * fr.ORACLE_TOL < fr.KERNEL_TOL, (ax, eu, ek)


def test_profile_holds_the_measured_tolerances():
    """profiles/fa_axis_parity.json (tools/fa_axis_parity.py): every non-default tolerance is TOL_FACTOR times the recorded
    oracle error, for every offset reducer set and every low-rank-kernel set."""
    rec = json.load(open(os.path.join(ROOT, "profiles", "fa_axis_parity.json")))
    names = [fr.reducer_name(*s) for s in fr.reducer_sets() if s[0] in fr.MEASURED_KINDS] + [fr.lrk_name(*s) for s in fr.lrk_sets()]
    assert rec["tol_factor"] == fr.TOL_FACTOR and rec["kernel_tol"] == fr.KERNEL_TOL
    for n in names:
        e = rec["sets"][n]
        assert e["tolerance"] == pytest.approx(fr.TOL_FACTOR * e["oracle_err"], rel=1e-12), n


# ---- the rotary table ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("freq", fr.FREQS)
def test_rotary_table_bit_for_bit(freq):
    """lns_rotary_table (the function a plan's tables come from) for n = 1 .. 200: every entry is float32(cos(float64(f))),
    float32(sin(float64(f))) of the float32 angle f built from torch.linspace positions.  numpy's float64 cosine and the C
    library's may differ in the last bit of the double; where float32 rounding would show that, the C library's value
    (math.cos) is the statement."""
    L = _L()
    DK = 128
    invf = np.ascontiguousarray(fr.inv_freq(freq, DK))
    half = DK // 2
    worst = 0.0
    for n in range(1, 201):
        out = np.full((half, n, 2), np.nan, np.float32)
        assert L.lns_rotary_table(n, invf.ctypes.data_as(ctypes.c_void_p), half, out.ctypes.data_as(ctypes.c_void_p)) == 0
        f = fr.rotary_angles(n, invf).astype(np.float64).T                    # [half, n]
        want = np.stack([np.cos(f), np.sin(f)], axis=-1).astype(np.float32)
        for d, i, k in zip(*np.nonzero(want.view(np.int32) != out.view(np.int32))):
            want[d, i, k] = np.float32((math.cos, math.sin)[k](f[d, i]))
        # (a torch whose linspace kernel contracts differently would fail here: rotary_table_fill follows torch 2.10's)
        assert np.array_equal(want.view(np.int32), out.view(np.int32)), (freq, n, "torch " + torch.__version__)
        worst = max(worst, float(f.max()))
    print("rotary table %s: n = 1 .. 200, DK = %d, largest angle %.1f rad: equal bits" % (freq, DK, worst))
    assert (worst > 600.0) == (freq == "x10")


def test_rotary_table_refuses_bad_arguments():
    from lns_amd import _lib
    L = _L()
    buf = (ctypes.c_float * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for args in ((0, p, 2, p), (4, None, 2, p), (4, p, 0, p), (4, p, 2, None)):
        assert L.lns_rotary_table(*args) == _lib.LNS_EINVAL, args


# ---- the fit predicates ----------------------------------------------------------------------------------------------------
def test_fit_predicates():
    """The LDS arithmetic of DESIGN.md "axis kernels: supported shapes", restated here, against the library's predicates on a
    grid around every limit; and the shapes every test of this pull request relies on."""
    L = _L()
    limit = 160 * 1024

    def mfma(C, Hid, Out):
        return C % 32 == 0 and Hid % 32 == 0 and C <= 256 and (max(C * Hid, 128 * Hid, 128 * Out) + 33 * (2 * C + Hid) + 256) * 4 <= limit

    def scalar(C, Hid, Out):
        return (C * C + C * Hid + Hid * Out + 16 * (2 * C + Hid)) * 4 <= limit
    for C in (1, 5, 24, 32, 40, 64, 96, 100, 128, 160, 256, 288):
        for Hid in (C, 2 * C, 2 * C + 1, 4 * C):
            for Out in (1, 16, 33, 64, 130, 200, 256, 300):
                assert L.lns_fa_reducer_fits(C, Hid, Out, 1) == int(mfma(C, Hid, Out)), (C, Hid, Out)
                assert L.lns_fa_reducer_fits(C, Hid, Out, 0) == int(mfma(C, Hid, Out) or scalar(C, Hid, Out)), (C, Hid, Out)
    assert (max(128 * 256, 128 * 256, 128 * 64) + 33 * 512 + 256) * 4 == 199680                                       # C = 128, MFMA form
    assert (128 * 128 + 128 * 256 + 256 * 64 + 16 * 512) * 4 == 294912                                                # its scalar form
    assert L.lns_fa_reducer_fits(128, 256, 64, 1) == 0 and L.lns_fa_reducer_fits(128, 256, 64, 0) == 0
    assert L.lns_fa_reducer_fits(256, 512, 64, 1) == 0 and L.lns_fa_reducer_fits(256, 512, 64, 0) == 0
    assert L.lns_fa_reducer_fits(96, 192, 64, 1) == 1
    for bad in ((0, 2, 2), (2, 0, 2), (2, 2, 0), (-32, 64, 32), (1 << 20, 1 << 20, 1 << 20)):
        assert L.lns_fa_reducer_fits(*bad, 0) == 0 and L.lns_fa_reducer_fits(*bad, 1) == 0, bad
    for s in fr.REDUCER_MFMA:
        assert L.lns_fa_reducer_fits(*s[2:], 1) == 1, s
    for s in fr.REDUCER_SCALAR:
        assert L.lns_fa_reducer_fits(*s[2:], 1) == 0 and L.lns_fa_reducer_fits(*s[2:], 0) == 1, s
    for DK in (2, 32, 64, 128, 256):
        for n in (1, 7, 32, 33, 64, 96, 128, 160, 161, 192, 320, 321, 700):
            assert L.lns_fa_lrk_fits(DK, n) == int(2 * DK * ((n + 31) // 32 * 32) * 4 <= limit), (DK, n)
    assert L.lns_fa_lrk_fits(128, 160) == 1 and 2 * 128 * 160 * 4 == limit and L.lns_fa_lrk_fits(128, 161) == 0
    for DK, n in ((127, 8), (0, 8), (-2, 8), (64, 0), (64, -1)):
        assert L.lns_fa_lrk_fits(DK, n) == 0, (DK, n)


# ---- argument checks, without a device -------------------------------------------------------------------------------------
def _host_ptr():
    buf = (ctypes.c_float * 16)()
    return ctypes.cast(buf, ctypes.c_void_p).value, buf


def _reducer_args(**over):
    """A two-axis call that passes every check; the pointers are host memory no check dereferences."""
    from lns_amd import _lib
    p, keep = _host_ptr()
    a = _lib.LnsFaReducerArgs()
    for name, _ in a._fields_:
        if name not in ("B", "nx", "ny", "C", "Hid", "Out", "form"):
            setattr(a, name, p)
    a.B, a.nx, a.ny, a.C, a.Hid, a.Out, a.form = 2, 7, 15, 64, 128, 64, 0
    for k, v in over.items():
        setattr(a, k, v)
    return a, keep


REDUCER_REFUSALS = [
    dict(mx=None), dict(ux=None), dict(to_in_x=None), dict(ln_g_x=None), dict(ln_b_x=None), dict(w1_x=None), dict(w2_x=None), dict(b2_x=None),
    dict(uy=None), dict(to_in_y=None), dict(ln_g_y=None), dict(ln_b_y=None), dict(w1_y=None), dict(w2_y=None), dict(b2_y=None),
    dict(my=None),                                   # form 0 with one axis
    dict(form=2), dict(form=-1),
    dict(B=0), dict(B=-1), dict(B=65536), dict(nx=0), dict(ny=0), dict(ny=65536),
    dict(C=128, Hid=256, Out=64), dict(C=128, Hid=256, Out=64, form=1), dict(C=256, Hid=512), dict(C=256, Hid=512, form=1),
    dict(C=24, Hid=48, Out=16),                      # the scalar form has no merged launch
    dict(C=0), dict(Hid=0), dict(Out=0), dict(Out=-4, form=1),
]


@pytest.mark.parametrize("over", REDUCER_REFUSALS, ids=lambda d: ",".join("%s=%s" % kv for kv in d.items()))
def test_reducer_refusals_precede_the_first_hip_call(over):
    from lns_amd import _lib
    L = _L()
    a, keep = _reducer_args(**over)
    assert L.lns_op_fa_reducer(ctypes.byref(a), None) == _lib.LNS_EINVAL, over
    assert L.lns_create_error().startswith(b"fa_reducer: "), L.lns_create_error()


def test_reducer_refusal_names_the_limit():
    from lns_amd import _lib
    L = _L()
    a, keep = _reducer_args(C=128, Hid=256, Out=64)
    assert L.lns_op_fa_reducer(ctypes.byref(a), None) == _lib.LNS_EINVAL
    msg = L.lns_create_error().decode()
    assert "C = 128" in msg and "199680" in msg and "294912" in msg and "163840" in msg, msg
    assert L.lns_op_fa_reducer(None, None) == _lib.LNS_EINVAL and L.lns_create_error().startswith(b"fa_reducer: ")


def _lrk_args(**over):
    from lns_amd import _lib
    p, keep = _host_ptr()
    a = _lib.LnsFaLrkArgs()
    a.qk_x = a.qk_y = a.inv_freq_x = a.inv_freq_y = a.kx = a.ky = p
    a.B_x = a.B_y = 2
    a.heads_x = a.heads_y = 2
    a.DK_x = a.DK_y = 64
    a.nx, a.ny, a.form = 7, 15, 0
    for k, v in over.items():
        setattr(a, k, v)
    return a, keep


LRK_REFUSALS = [
    dict(qk_x=None), dict(inv_freq_x=None), dict(kx=None), dict(inv_freq_y=None), dict(ky=None),
    dict(qk_y=None),                                 # form 0 with one axis
    dict(form=2), dict(form=-1),
    dict(B_x=0, B_y=0), dict(B_x=65536, B_y=65536), dict(heads_x=0, heads_y=0), dict(heads_x=65536, heads_y=65536),
    dict(B_y=0, form=1), dict(heads_y=-1, form=1),
    dict(DK_x=63, DK_y=63), dict(DK_y=33, form=1), dict(DK_x=0, DK_y=0),
    dict(B_y=3), dict(heads_y=4), dict(DK_y=32),     # the two axes differ in a merged launch
    dict(nx=0), dict(ny=-2),
    dict(DK_x=128, DK_y=128, ny=161), dict(DK_x=128, nx=161, form=1), dict(DK_x=128, DK_y=128, nx=161, ny=8),
]


@pytest.mark.parametrize("over", LRK_REFUSALS, ids=lambda d: ",".join("%s=%s" % kv for kv in d.items()))
def test_lrk_refusals_precede_the_first_hip_call(over):
    from lns_amd import _lib
    L = _L()
    a, keep = _lrk_args(**over)
    assert L.lns_op_fa_lrk(ctypes.byref(a), None) == _lib.LNS_EINVAL, over
    assert L.lns_create_error().startswith(b"fa_lrk: "), L.lns_create_error()
    assert L.lns_op_fa_lrk(None, None) == _lib.LNS_EINVAL and L.lns_create_error().startswith(b"fa_lrk: ")


def test_build_advertises_the_entry_points():
    assert _L().lns_build_has(b"op_fa_axis") == 1

"""GPU: ln_pe_kernel (the SABlock pre-norm) and apply_kernel (a pending GroupNorm + activation materialised) at op level
through lns_op_ln_pe / lns_op_apply, against the float64 statements of tests/fa_axis_reference.py.  KERNEL_TOL = 2e-6,
relative L2 per sample.  Outputs are pre-filled with NaN and followed by 64 canary floats.

ln_pe   six shapes, C = 160 and 256 on the kernel's loop path (C / 4 > 32), n not a multiple of the 64-token block; rows with
        a per-channel offset and one one-hot token per sample; with and without pe, whose table has more rows than there are
        tokens; samples C n + 37 floats apart give the bits of the contiguous run; max |h| stays below the bound the planner
        hands the consumer (bound_out), which is the float32 value of sqrt(C) max|gamma| + max|beta| + max|pe|.
apply   every activation 0..5 at HW = 1, 105, 256, 4097, with and without a (scale, shift) table, contiguous and with samples
        further apart (same bits), inputs of magnitude 1e-20, 1 and 1e20 with finite outputs; amax_out is the bit pattern of
        max |y| of the stored sample, exactly.

Measured on an MI355X: ln_pe 6.0e-8 .. 8.7e-8 (max |h| 0.89 .. 0.997 of bound_out); apply at most 5.6e-8 (gelu), 0 at 1e20
where the activation saturates.  The file: 31 tests, 1 s."""
import ctypes

import numpy as np
import pytest
import torch

import fa_axis_reference as fr

pytestmark = pytest.mark.gpu

NAN = float("nan")
CANARY, CANARY_VALUE = 64, -7.25
PAD = 37


def _L():
    from lns_amd import _lib
    assert torch.cuda.is_available(), "GPU test selected but no GPU is visible"
    L = _lib.lib()
    assert L.lns_build_has(b"op_fa_axis") == 1
    return L


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _hp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def guarded(n):
    buf = torch.full((n + CANARY,), NAN, dtype=torch.float32, device="cuda")
    buf[n:] = CANARY_VALUE
    return buf


def read_guarded(buf, shape, what):
    host = buf.cpu().numpy()
    n = int(np.prod(shape))
    assert (host[n:] == CANARY_VALUE).all(), "%s: a canary behind the output was written" % what
    assert not np.isnan(host[:n]).any(), "%s: unwritten outputs" % what
    return host[:n].reshape(shape)


def strided(x, pad):
    """x [B, ...] on the device with samples `pad` floats further apart than they are long (NaN in between)."""
    B, per = x.shape[0], int(np.prod(x.shape[1:]))
    buf = np.full((B, per + pad), np.nan, np.float32)
    buf[:, :per] = x.reshape(B, per)
    return torch.from_numpy(buf).cuda(), per + pad


def _rc(rc, what):
    from lns_amd import _lib
    if rc == _lib.LNS_EHIP:                 # a HIP error: nothing more is started on this device
        pytest.exit("%s: HIP error" % what, returncode=3)
    torch.cuda.synchronize()
    assert rc == 0, (what, rc, _lib.lib().lns_create_error().decode())


def run_ln_pe(r, with_pe, pad=0):
    L = _L()
    B, C, n = r["B"], r["C"], r["n"]
    xd, x_bs = strided(r["x"], pad)
    g, be, pe = (np.ascontiguousarray(r[k]) for k in ("gamma", "beta", "pe"))
    h = guarded(B * C * n)
    bound = ctypes.c_float(NAN)
    what = "lns_op_ln_pe (%d, %d, %d) pe=%d pad=%d" % (B, C, n, with_pe, pad)
    _rc(L.lns_op_ln_pe(xd.data_ptr(), x_bs, B, C, n, _hp(g), _hp(be), _hp(pe) if with_pe else None, pe.shape[0] if with_pe else 0,
                       fr.LN_EPS, h.data_ptr(), ctypes.byref(bound), _stream()), what)
    return read_guarded(h, (B, C, n), what), bound.value


@pytest.mark.parametrize("shape", fr.LNPE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ln_pe_parity_bound_and_stride(shape):
    r = fr.lnpe_set(*shape)
    B, C, n = shape
    for with_pe in (False, True):
        h, bound = run_ln_pe(r, with_pe)
        err = fr.rel_l2(h, r["ref"][with_pe], 1)
        want = fr.lnpe_bound(C, r["gamma"], r["beta"], r["pe"] if with_pe else None)
        print("ln_pe %s pe=%d: rel-L2 per sample, worst %.2e; max |h| %.5f, bound_out %.5f" % (shape, with_pe, err.max(), np.abs(h).max(), bound))
        assert np.isfinite(h).all() and (err <= fr.KERNEL_TOL).all(), (shape, with_pe, err)
        assert np.abs(h).max() <= bound, (shape, with_pe, np.abs(h).max(), bound)
        assert abs(bound - want) <= 4 * np.spacing(np.float32(want)), (bound, want)       # three float32 operations
        h2, bound2 = run_ln_pe(r, with_pe, pad=PAD)
        assert np.array_equal(h.view(np.int32), h2.view(np.int32)) and bound2 == bound, (shape, with_pe, "x_bs = C n + 37")


def run_apply(x, ss, act, pad=0):
    L = _L()
    B, C, HW = x.shape
    xd, x_bs = strided(x, pad)
    ssd = torch.from_numpy(ss).cuda() if ss is not None else None
    y = guarded(B * C * HW)
    amax = torch.zeros((B * 16 + CANARY,), dtype=torch.int32, device="cuda")
    amax[B * 16:] = 0x5A5A5A5A
    what = "lns_op_apply (%d, %d, %d) act %d ss=%d pad=%d" % (B, C, HW, act, ss is not None, pad)
    _rc(L.lns_op_apply(xd.data_ptr(), x_bs, ssd.data_ptr() if ssd is not None else None, act, B, C, HW, y.data_ptr(), amax.data_ptr(),
                       _stream()), what)
    words = amax.cpu().numpy()
    assert (words[B * 16:] == 0x5A5A5A5A).all(), what + ": a canary behind amax_out was written"
    return read_guarded(y, (B, C, HW), what), words[:B * 16].reshape(B, 16).max(axis=1).view(np.float32)


@pytest.mark.parametrize("HW", fr.APPLY_HW)
@pytest.mark.parametrize("act", range(6))
def test_apply_parity_amax_and_stride(act, HW):
    B, C = 2, 3
    for mag in fr.APPLY_MAGS:
        x, ss = fr.apply_input(B, C, HW, mag)
        for table in (None, ss):
            y, amax = run_apply(x, table, act)
            ref = fr.apply64(x, table, act)
            assert np.isfinite(y).all(), (act, HW, mag, "non-finite outputs")
            if np.any(ref):
                err = fr.rel_l2(y, ref, 1)
                print("apply act %d HW %d |x| ~ %g ss=%d: rel-L2 per sample, worst %.2e" % (act, HW, mag, table is not None, err.max()))
                assert (err <= fr.KERNEL_TOL).all(), (act, HW, mag, table is not None, err)
            else:
                assert not np.any(y)
            want = np.abs(y).reshape(B, -1).max(axis=1)
            assert np.array_equal(amax.view(np.int32), want.view(np.int32)), (act, HW, mag, "amax", amax, want)
            y2, amax2 = run_apply(x, table, act, pad=PAD)
            assert np.array_equal(y.view(np.int32), y2.view(np.int32)) and np.array_equal(amax.view(np.int32), amax2.view(np.int32))


def test_apply_without_amax_out():
    from lns_amd import _lib
    L = _L()
    x, ss = fr.apply_input(2, 3, 105, 1.0)
    xd, ssd, y = torch.from_numpy(x).cuda(), torch.from_numpy(ss).cuda(), guarded(x.size)
    _rc(L.lns_op_apply(xd.data_ptr(), 3 * 105, ssd.data_ptr(), 2, 2, 3, 105, y.data_ptr(), None, _stream()), "lns_op_apply amax_out = NULL")
    got = read_guarded(y, x.shape, "lns_op_apply amax_out = NULL")
    assert np.array_equal(got.view(np.int32), run_apply(x, ss, 2)[0].view(np.int32))

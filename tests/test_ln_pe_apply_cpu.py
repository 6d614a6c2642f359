"""CPU: the float64 statements of ln_pe and apply (tests/fa_axis_reference.py) against the float32 oracle on the input sets of
tests/test_ln_pe_apply_gpu.py, the planner's bound of the ln_pe output on its extremal input, and the argument checks of
lns_op_ln_pe / lns_op_apply, which precede the first HIP call and need no device."""
import ctypes

import numpy as np
import pytest

import fa_axis_reference as fr


def _L():
    from lns_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("shape", fr.LNPE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ln_pe_statement_agrees_with_the_oracle(shape):
    """lns_oracle.layernorm (+ pe) within ORACLE_TOL per sample, offsets and one-hot tokens included; the one-hot token sits
    at sqrt(C - 1) |gamma| + beta (+ pe) and the bound sqrt(C) max|gamma| + max|beta| + max|pe| holds, closely for sample 0."""
    r = fr.lnpe_set(*shape)
    B, C, n = shape
    for with_pe in (False, True):
        pe = r["pe"] if with_pe else None
        err = fr.rel_l2(fr.lnpe_oracle(r["x"], r["gamma"], r["beta"], pe), r["ref"][with_pe], 1)
        bound = fr.lnpe_bound(C, r["gamma"], r["beta"], pe)
        top = np.abs(r["ref"][with_pe]).max()
        print("ln_pe %s pe=%d: oracle rel-L2 per sample, worst %.2e; max |h| %.4f of the bound %.4f" % (shape, with_pe, err.max(), top, bound))
        assert err.max() < fr.ORACLE_TOL
        reach = np.sqrt(C - 1.0) * 0.999 * np.abs(r["gamma"]).max() - np.abs(r["beta"]).max() - (np.abs(pe).max() if with_pe else 0.0)
        assert reach <= top <= bound, (reach, top, bound)
    for b, i in enumerate(fr.hot_tokens(B, n)):
        assert np.count_nonzero(r["x"][b, :, i]) == 1
    assert r["pe"].shape == (n + 11, C)


@pytest.mark.parametrize("act", range(6))
def test_apply_statement_agrees_with_the_oracle(act):
    """The oracle's activations at magnitude 1 within ORACLE_TOL; the statement is finite at 1e-20 and 1e20 for every
    activation."""
    import lns_oracle
    for HW in fr.APPLY_HW:
        for mag in fr.APPLY_MAGS:
            x, ss = fr.apply_input(2, 3, HW, mag)
            for table in (None, ss):
                ref = fr.apply64(x, table, act)
                assert np.isfinite(ref).all(), (act, HW, mag)
                if mag == 1.0 and HW > 1:
                    v = x if table is None else (x * table[..., 0:1] + table[..., 1:2]).astype(np.float32)
                    o = v if act == 0 else lns_oracle.activation(v, ("", "silu", "gelu", "relu", "tanh", "sigmoid")[act])
                    err = fr.rel_l2(o, ref, 1)
                    assert err.max() < fr.ORACLE_TOL, (act, HW, err)


def _p():
    buf = (ctypes.c_float * 16)()
    return ctypes.cast(buf, ctypes.c_void_p), buf


def _ln_pe(**over):
    """lns_op_ln_pe's arguments, by name, of a call that passes every check."""
    p, keep = _p()
    a = dict(x=p, x_bs=30 * 70, B=3, C=30, n=70, gamma=p, beta=p, pe=p, pe_len=81, eps=1e-5, h=p, bound=None, stream=None)
    a.update(over)
    return list(a.values()), keep


@pytest.mark.parametrize("over", [dict(x=None), dict(h=None), dict(gamma=None), dict(beta=None), dict(B=0), dict(B=65536), dict(C=0),
                                  dict(n=0), dict(x_bs=30 * 70 - 1), dict(x_bs=0), dict(pe_len=69), dict(eps=0.0), dict(eps=-1e-5),
                                  dict(eps=float("nan")), dict(C=1 << 16, n=1 << 15, x_bs=1 << 40)],
                         ids=lambda d: ",".join("%s=%s" % kv for kv in d.items()))
def test_ln_pe_refusals_precede_the_first_hip_call(over):
    from lns_amd import _lib
    L = _L()
    args, keep = _ln_pe(**over)
    assert L.lns_op_ln_pe(*args) == _lib.LNS_EINVAL, over
    assert L.lns_create_error().startswith(b"ln_pe: "), L.lns_create_error()


def _apply(**over):
    p, keep = _p()
    a = dict(x=p, x_bs=3 * 105, ss=None, act=2, B=2, C=3, HW=105, y=p, amax=None, stream=None)
    a.update(over)
    return list(a.values()), keep


@pytest.mark.parametrize("over", [dict(x=None), dict(y=None), dict(act=-1), dict(act=6), dict(B=0), dict(B=65536), dict(C=0), dict(HW=0),
                                  dict(x_bs=3 * 105 - 1), dict(x_bs=-1), dict(C=1 << 16, HW=1 << 15, x_bs=1 << 40)],
                         ids=lambda d: ",".join("%s=%s" % kv for kv in d.items()))
def test_apply_refusals_precede_the_first_hip_call(over):
    from lns_amd import _lib
    L = _L()
    args, keep = _apply(**over)
    assert L.lns_op_apply(*args) == _lib.LNS_EINVAL, over
    assert L.lns_create_error().startswith(b"apply: "), L.lns_create_error()

"""GPU: the elementwise and reduction kernels of the training rollout's backward pass on their own (lns_op_groupnorm_train,
lns_op_gelu_grad, lns_op_bias_grad: the rollout's launchers behind thin entry points), against float64 torch on the CPU, on
the inputs a randomly initialised network never produces: a constant group, a large mean over a small spread, a saturated
GELU, an accumulate flag over existing contents.

Tolerance: KERNEL_TOL of tests/test_gpu_parity.py (rel-L2 per output tensor).  Where a case is ill-conditioned by
construction the bound is max(KERNEL_TOL, 3 x the error of torch's own float32 CPU op against float64); each such case says
so where it is defined."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

KERNEL_TOL = 2e-6          # tests/test_gpu_parity.py


def _need_gpu():
    assert torch.cuda.is_available(), "GPU test selected but no GPU is visible"


def _L():
    from lns_amd import _lib
    L = _lib.lib()
    assert L.lns_build_has(b"train_ops") == 1
    return L


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    den = np.sqrt((b ** 2).sum())
    if den == 0.0:
        return float(np.sqrt(((a - b) ** 2).sum()))       # an exactly zero expectation: absolute
    return float(np.sqrt(((a - b) ** 2).sum()) / den)


# ---- GroupNorm, training form ---------------------------------------------------------------------------------------
GN_SHAPES = [(1, 32, 1, 32), (3, 160, 63, 32), (2, 96, 65, 32), (2, 64, 257, 1), (5, 128, 64, 1)]     # (B, C, HW, groups)
# input kinds.  A case is held to KERNEL_TOL alone unless it is ill-conditioned by construction (`_gn_ill`); then the bound
# is max(KERNEL_TOL, 3 x the error of torch's own float32 CPU op against float64).
#   random      N(0.7, 1.5), the distribution of the existing GroupNorm test
#   const_group one group of every sample holds a single value (with one group: the whole sample): variance exactly 0,
#               rstd = 1 / sqrt(eps), xhat = 0.  Not ill: the sum of n equal values 3.25 is exact in float32 for these n
#   big_mean    mean 1e3, spread 1e-2.  ILL: x - mean is taken from a mean rounded to 2^-24 * 1e3 = 6e-5, 6e-3 of the
#               spread, which no implementation that keeps a float32 mean can undo
#   gamma_zero  gamma = 0 on every third channel (dx of those channels' share and their y = beta exactly)
#   dy_zero     dy = 0: dx = add (or 0), dgamma = dbeta = 0 exactly
# The shape (1, 32, 1, 32) is ILL under every kind: each group holds one value, so dx = rstd (gamma dy - mean_g(gamma dy))
# is a complete cancellation whose exact value is add (or 0); what an implementation returns is its rounding residue of
# terms of size rstd |gamma dy| = 1e3 |gamma dy|.
GN_KINDS = ("random", "const_group", "big_mean", "gamma_zero", "dy_zero")


def _gn_ill(shape, kind):
    B, C, HW, groups = shape
    return kind == "big_mean" or (C // groups) * HW == 1


def _gn_inputs(B, C, HW, groups, kind, seed):
    r = np.random.default_rng(seed)
    x = (r.standard_normal((B, C, HW)) * 1.5 + 0.7).astype(np.float32)
    gamma = (1 + 0.1 * r.standard_normal(C)).astype(np.float32)
    beta = (0.1 * r.standard_normal(C)).astype(np.float32)
    dy = r.standard_normal((B, C, HW)).astype(np.float32)
    add = r.standard_normal((B, C, HW)).astype(np.float32)
    cg = C // groups
    if kind == "const_group":
        g = groups // 2
        x[:, g * cg:(g + 1) * cg, :] = np.float32(3.25)
    elif kind == "big_mean":
        x = (1e3 + 1e-2 * r.standard_normal((B, C, HW))).astype(np.float32)
    elif kind == "gamma_zero":
        gamma[::3] = 0.0
    elif kind == "dy_zero":
        dy[:] = 0.0
    return x, gamma, beta, dy, add


def _gn_torch(x, gamma, beta, dy, add, groups, eps, dtype):
    if x.shape[0] * x.shape[2] == 1:
        # F.group_norm refuses a single value per channel (B * HW = 1).  GroupNorm is per sample: the same op on the
        # sample twice, the copy with dy = 0 (nothing of it reaches dgamma / dbeta), and the first sample's results
        r = _gn_torch(np.concatenate([x, x]), gamma, beta, np.concatenate([dy, np.zeros_like(dy)]),
                      None if add is None else np.concatenate([add, add]), groups, eps, dtype)
        return {k: (v if k in ("dgamma", "dbeta") else v[:1]) for k, v in r.items()}
    xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
    gt = torch.from_numpy(gamma).to(dtype).requires_grad_(True)
    bt = torch.from_numpy(beta).to(dtype).requires_grad_(True)
    y = F.group_norm(xt, groups, gt, bt, eps)
    y.backward(torch.from_numpy(dy).to(dtype))
    B, C, HW = x.shape
    xg = xt.detach().reshape(B, groups, -1)
    mean = xg.mean(-1)
    rstd = 1.0 / torch.sqrt(xg.var(-1, unbiased=False) + eps)
    dx = xt.grad if add is None else xt.grad + torch.from_numpy(add).to(dtype)
    return dict(y=y.detach().numpy(), mean=mean.numpy(), rstd=rstd.numpy(), dx=dx.numpy(), dgamma=gt.grad.numpy(),
                dbeta=bt.grad.numpy())


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("kind", sorted(GN_KINDS))
@pytest.mark.parametrize("shape", GN_SHAPES, ids=lambda s: "B%d-C%d-HW%d-G%d" % s)
def test_groupnorm_train(shape, kind, with_add, accumulate):
    """Forward (y, mean, rstd) and backward (dx with the optional skip gradient, dgamma / dbeta through colsum2 with the
    accumulate flag over non-zero contents).  (3, 160, 63, 32) has 5 channels per group: the per-channel partial loop of the
    backward kernel takes its second pass; 63 / 65 / 257 pixels are ragged against the 64-lane and 256-thread strides."""
    _need_gpu()
    L = _L()
    B, C, HW, groups = shape
    eps = 1e-6 if groups == 32 else 1e-5
    x, gamma, beta, dy, add = _gn_inputs(B, C, HW, groups, kind, seed=B * 1000 + C + HW)
    addv = add if with_add else None
    ref = _gn_torch(x, gamma, beta, dy, addv, groups, eps, torch.float64)
    r32 = _gn_torch(x, gamma, beta, dy, addv, groups, eps, torch.float32)
    if (C // groups) * HW == 1:
        # every group holds a single value: dx = add (or 0) in exact arithmetic.  float64 torch keeps its own residue of the
        # cancellation (1e-13 of the cancelling terms), so the analytic answer is the expectation, for the kernel and for
        # torch's float32 op alike (`_rel` is absolute where the expectation is exactly zero)
        for rr in (ref, r32):
            rr["dx"] = (add if with_add else np.zeros_like(add)).astype(np.float64)
    r = np.random.default_rng(7)
    dg0 = r.standard_normal(C).astype(np.float32)           # what dgamma / dbeta hold before the call
    db0 = r.standard_normal(C).astype(np.float32)
    if accumulate:
        ref["dgamma"] = ref["dgamma"] + dg0
        ref["dbeta"] = ref["dbeta"] + db0
        r32["dgamma"] = r32["dgamma"] + dg0
        r32["dbeta"] = r32["dbeta"] + db0
    xd, gd, bd, dyd = _dev(x), _dev(gamma), _dev(beta), _dev(dy)
    addd = _dev(add) if with_add else None
    nan = float("nan")
    y = torch.full((B, C, HW), nan, dtype=torch.float32, device="cuda")
    stats = torch.full((B, groups, 2), nan, dtype=torch.float32, device="cuda")
    dx = torch.full((B, C, HW), nan, dtype=torch.float32, device="cuda")
    part = torch.full((B, C, 2), nan, dtype=torch.float32, device="cuda")
    dgd, dbd = _dev(dg0), _dev(db0)
    rc = L.lns_op_groupnorm_train(xd.data_ptr(), B, C, HW, groups, eps, gd.data_ptr(), bd.data_ptr(), y.data_ptr(), stats.data_ptr(),
                                  dyd.data_ptr(), addd.data_ptr() if with_add else None, dx.data_ptr(), dgd.data_ptr(), dbd.data_ptr(),
                                  accumulate, part.data_ptr(), _stream())
    assert rc == 0, L.lns_create_error().decode()
    st = stats.cpu().numpy()
    got = dict(y=y.cpu().numpy(), mean=st[..., 0], rstd=st[..., 1], dx=dx.cpu().numpy(), dgamma=dgd.cpu().numpy(), dbeta=dbd.cpu().numpy())
    for k in ("y", "mean", "rstd", "dx", "dgamma", "dbeta"):
        assert np.isfinite(got[k]).all(), k
        own = _rel(r32[k], ref[k]) if _gn_ill(shape, kind) else 0.0
        err = _rel(got[k], ref[k])
        print("gn", shape, kind, with_add, accumulate, k, "err %.3e own %.3e" % (err, own))
        assert err <= max(KERNEL_TOL, 3.0 * own), (k, err, own)
    if kind == "dy_zero":                                    # exact: nothing but the skip gradient and the old contents
        assert np.array_equal(got["dx"], add if with_add else np.zeros_like(add))
        assert np.array_equal(got["dgamma"], dg0 if accumulate else np.zeros_like(dg0))
        assert np.array_equal(got["dbeta"], db0 if accumulate else np.zeros_like(db0))
    if kind == "gamma_zero":
        assert np.array_equal(got["y"][:, ::3], np.broadcast_to(beta[::3][None, :, None], got["y"][:, ::3].shape))


def test_groupnorm_train_refuses_bad_arguments():
    """Host-side checks come before any launch: a group count that does not divide C, a backward without its buffers."""
    _need_gpu()
    L = _L()
    t = torch.zeros(64, dtype=torch.float32, device="cuda")
    p = t.data_ptr()
    assert L.lns_op_groupnorm_train(p, 1, 6, 1, 4, 1e-5, p, p, p, p, None, None, None, None, None, 0, None, _stream()) == -1
    assert b"divisor" in L.lns_create_error()
    assert L.lns_op_groupnorm_train(p, 1, 4, 1, 2, 1e-5, p, p, p, p, p, None, None, p, p, 0, p, _stream()) == -1
    assert L.lns_op_gelu_grad(p, p, p, 0, _stream()) == -1
    assert L.lns_op_bias_grad(p, 1, 1, 1, p, 2, _stream()) == -1


# ---- GELU gradient --------------------------------------------------------------------------------------------------
GELU_N = [1, 255, 256, 257, 2048 * 256 + 3]      # below / at / above one block; past the 2048-block grid cap (a second trip)
GELU_U = [0.0, 1e-8, 0.5, 3.0, 6.0, 12.0, 40.0]


def _gelu_grad_torch(u, dy, dtype):
    ut = torch.from_numpy(u).to(dtype).requires_grad_(True)
    F.gelu(ut).backward(torch.from_numpy(dy).to(dtype))
    return ut.grad.numpy()


def _gelu_run(u, dy):
    L = _L()
    ud, dyd = _dev(u), _dev(dy)
    du = torch.full((u.size,), float("nan"), dtype=torch.float32, device="cuda")
    rc = L.lns_op_gelu_grad(dyd.data_ptr(), ud.data_ptr(), du.data_ptr(), u.size, _stream())
    assert rc == 0, L.lns_create_error().decode()
    return du.cpu().numpy()


@pytest.mark.parametrize("n", GELU_N)
def test_gelu_grad_finite_domain(n):
    """u cycles through +-{0, 1e-8, 0.5, 3, 6, 12, 40} (the saturated tails included: Phi = 0 or 1, u phi(u) underflows),
    then random values; every element against float64.  Besides the rel-L2 bound every element is within KERNEL_TOL
    of the largest expected magnitude: the derivative is O(1) and float32 forms Phi from 1 + erf, so the tails are
    exact to 2^-24 of one, not of themselves."""
    _need_gpu()
    pts = np.array([s * v for v in GELU_U for s in (1.0, -1.0)], np.float32)
    r = np.random.default_rng(n)
    u = np.resize(pts, n).astype(np.float32)
    if n > 2 * pts.size:
        u[2 * pts.size:] = (3.0 * r.standard_normal(n - 2 * pts.size)).astype(np.float32)
    dy = (0.5 + r.random(n)).astype(np.float32) * np.where(r.random(n) < 0.5, -1.0, 1.0).astype(np.float32)
    ref = _gelu_grad_torch(u, dy, torch.float64)
    got = _gelu_run(u, dy)
    assert np.isfinite(got).all()
    err = _rel(got, ref)
    print("gelu n=%d err %.3e" % (n, err))
    assert err <= KERNEL_TOL, (n, err)
    assert (np.abs(got - ref) <= KERNEL_TOL * np.abs(ref).max()).all()


def test_gelu_grad_nonfinite_inputs_follow_torch():
    """u = +-inf and NaN, by class against torch's own float32 gelu backward on the CPU: the same finite value, an
    infinity of the same sign, or NaN where torch gives NaN."""
    _need_gpu()
    u = np.array([np.inf, -np.inf, np.nan, 1.0, np.inf, -np.inf], np.float32)
    dy = np.array([1.0, 1.0, 1.0, np.nan, -2.0, 0.0], np.float32)
    want = _gelu_grad_torch(u, dy, torch.float32)
    got = _gelu_run(u, dy)
    for i in range(u.size):
        if np.isnan(want[i]):
            assert np.isnan(got[i]), (i, u[i], dy[i], got[i], want[i])
        elif np.isinf(want[i]):
            assert np.isinf(got[i]) and np.sign(got[i]) == np.sign(want[i]), (i, u[i], dy[i], got[i], want[i])
        else:
            assert abs(got[i] - want[i]) <= KERNEL_TOL * max(1.0, abs(want[i])), (i, u[i], dy[i], got[i], want[i])


# ---- bias gradient --------------------------------------------------------------------------------------------------
BIAS_SHAPES = [(1, 1, 1), (3, 5, 63), (33, 16, 64), (2, 64, 257)]     # (B, C, HW)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("shape", BIAS_SHAPES, ids=lambda s: "B%d-C%d-HW%d" % s)
def test_bias_grad(shape, accumulate):
    """db[c] (+)= sum over batch and pixels, against float64, over non-zero contents; two runs give the same bits.
    dy has mean 0.3, so the sum is not a cancellation and KERNEL_TOL holds as it stands."""
    _need_gpu()
    L = _L()
    B, C, HW = shape
    r = np.random.default_rng(B + C + HW)
    dy = (r.standard_normal((B, C, HW)) + 0.3).astype(np.float32)
    db0 = r.standard_normal(C).astype(np.float32)
    ref = dy.astype(np.float64).sum((0, 2)) + (db0 if accumulate else 0.0)
    dyd = _dev(dy)
    outs = []
    for _ in range(2):
        db = _dev(db0)
        rc = L.lns_op_bias_grad(dyd.data_ptr(), B, C, HW, db.data_ptr(), accumulate, _stream())
        assert rc == 0, L.lns_create_error().decode()
        outs.append(db.cpu().numpy())
    assert np.array_equal(outs[0], outs[1])
    # per element: a sum of n terms of magnitude ~1 carries n-independent relative rounding only against sum |dy|
    scale = np.abs(dy.astype(np.float64)).sum((0, 2)) + np.abs(db0)
    assert (np.abs(outs[0] - ref) <= KERNEL_TOL * scale).all(), (np.abs(outs[0] - ref) / scale).max()
    assert _rel(outs[0], ref) <= KERNEL_TOL, _rel(outs[0], ref)

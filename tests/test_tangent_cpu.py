"""CPU: the tangent-linear rollout (include/lns.h "tangent-linear rollout").

  * the reference (tests/tangent_reference.py) checks itself: forward-mode autograd against a central difference, against
    reverse-mode autograd through <J v, w> = <v, J^T w>, the hand-written tangent against forward-mode autograd, the
    Gram-Schmidt statement against torch.linalg.qr;
  * the inputs of the GPU grid tell every deliberate mistake of a hand-written JVP from the truth by 100x the GPU tolerance;
  * lns_train_tangent, its size query and lns_op_orthonormalize are declared, exported and announced, size the workspace by
    the documented layout without a GPU, and refuse bad arguments in the documented order (fake pointers, no device here);
  * TangentRollout.lyapunov refuses bad arguments before any device work."""
import ctypes
import os
import re

import pytest
import torch

import latent_fit_reference as lf
import tangent_reference as tg
import train_reference as tr
from helpers import ROOT

SYMBOLS = ("lns_train_tangent_workspace_bytes", "lns_train_tangent", "lns_op_orthonormalize")
P = ctypes.c_void_p(0x1000)


@pytest.fixture(autouse=True, scope="module")
def _feature_is_built():
    """The reference's self-checks below license the GPU tests of a feature: without it in the library they say nothing."""
    from lns_amd import _lib
    _lib.build()
    assert _lib.lib().lns_build_has(b"rollout_tangent") == 1


def _engine(preset="ns2d_mini", **kw):
    from lns_amd import config, engine
    a = config.preset(preset)
    return engine.Engine(engine.make_config(a, ae_prefix="ae." if a.family == "twophase_cond" else "vq_ae.",
                                            prop_prefix="propagator.", **kw))


def _params(e, fake=0x1000):
    a = (ctypes.c_void_p * len(e.params))()
    for i, (k, _, isb) in enumerate(e.params):
        if k.startswith("propagator.") and not isb:
            a[i] = fake
    return a


def _round256(n):
    return -(-n // 256) * 256


# ---- the reference checks itself ------------------------------------------------------------------------------------------
CHECK = [(("E3", 2, 2, 4, 4), 2), (("E1", 2, 1, 3, 5), 1), (("E5", 2, 2, 2, 2), 3), (("E6", 2, 2, 7, 15), 2)]


def _f64_problem(case, K):
    z0, prm, v = tg.case_start(case, K)
    return lf.propagator(case[0]), lf.t64(z0), lf.t64(prm), lf.t64(v)


@pytest.mark.parametrize("g", CHECK, ids=tg.grid_id)
def test_float64_jvp_is_the_derivative(g):
    """Forward-mode autograd against (f(z + h v) - f(z - h v)) / 2h, h = 1e-5, float64: truncation ~ h^2 |f'''|, rounding
    ~ 1e-16 / h.  Measured: 3.9e-10 .. 1.5e-9 rel-L2 over the four cases; asserted 1e-7."""
    case, K = g
    prop, z0, prm, v = _f64_problem(case, K)
    T, h = case[2], 1e-5
    with torch.no_grad():
        _, jv = tg.jvp_rollout(prop, z0, prm, v, T)
        for k in range(K):
            fd = (lf.rollout(prop, z0 + h * v[:, k], prm, T) - lf.rollout(prop, z0 - h * v[:, k], prm, T)) / (2 * h)
            err = tr.rel_l2(jv[:, k].numpy(), fd.numpy())
            print(tg.grid_id(g), "k", k, "jvp vs central difference rel-L2 %.3g" % err)
            assert err < 1e-7, err


@pytest.mark.parametrize("g", CHECK, ids=tg.grid_id)
def test_float64_jvp_pairs_with_autograd_vjp(g):
    """<J v, w> = <v, J^T w>, J^T w by reverse-mode autograd: measured 3.6e-17 .. 4.1e-16 of |J v| |w|; asserted 1e-13.
    The hand-written tangent (no variant) is forward-mode autograd: measured <= 3.3e-15 rel-L2 on the grid; asserted 1e-13."""
    case, K = g
    prop, z0, prm, v = _f64_problem(case, K)
    B, T = case[1], case[2]
    with torch.no_grad():
        _, jv = tg.jvp_rollout(prop, z0, prm, v, T)
        _, mv = tg.manual_jvp_rollout(prop, z0, prm, v, T)
    assert tr.rel_l2(mv.numpy(), jv.numpy()) < 1e-13
    w = lf.t64(tg.orth_input((B,) + tuple(z0.shape[1:]), seed=5))
    z = z0.clone().requires_grad_(True)
    (lf.rollout(prop, z, prm, T)[:, -1] * w).sum().backward()
    for k in range(K):
        lhs = (jv[:, k, -1] * w).reshape(B, -1).sum(1)
        rhs = (v[:, k] * z.grad).reshape(B, -1).sum(1)
        scale = jv[:, k, -1].reshape(B, -1).norm(dim=1) * w.reshape(B, -1).norm(dim=1)
        rel = ((lhs - rhs).abs() / scale).max().item()
        print(tg.grid_id(g), "k", k, "dot-product defect %.3g" % rel)
        assert rel < 1e-13, rel


@pytest.mark.parametrize("shape", [s for s in tg.ORTH_SHAPES if s[1] <= s[2]], ids=str)
def test_mgs_statement_is_a_qr_factorisation(shape):
    """float64 MGS against torch.linalg.qr with the signs fixed (R_kk > 0).  Measured on N(0,1): Q 1.8e-16 .. 1.7e-15, R
    9.0e-17 .. 4.7e-16 rel-L2 ((2,32,32), K = n, is the worst conditioned); asserted 1e-12."""
    V = lf.t64(tg.orth_input(shape))
    Q, R, logr = tg.mgs(V)
    q, r = torch.linalg.qr(V.transpose(1, 2))                       # [B,n,K], [B,K,K]
    s = torch.sign(torch.diagonal(r, dim1=1, dim2=2))
    q, r = q * s[:, None, :], r * s[:, :, None]
    eq, er = tr.rel_l2(Q.numpy(), q.transpose(1, 2).numpy()), tr.rel_l2(R.numpy(), r.numpy())
    print(shape, "Q %.3g R %.3g" % (eq, er))
    assert eq < 1e-12 and er < 1e-12
    assert torch.equal(logr, torch.log(torch.diagonal(R, dim1=1, dim2=2)))
    assert (torch.tril(R, -1) == 0).all()


def test_mgs_statement_on_a_zero_vector():
    V = lf.t64(tg.orth_input((2, 3, 32)))
    V[:, 1] = 0
    for dtype in (torch.float64, torch.float32):
        Q, R, logr = tg.mgs(V, dtype)
        assert not torch.isnan(Q).any() and (Q[:, 1] == 0).all()
        assert torch.isinf(logr[:, 1]).all() and (logr[:, 1] < 0).all() and torch.isfinite(logr[:, [0, 2]]).all()


# ---- the GPU grid tells mistakes from the truth -----------------------------------------------------------------------------
@pytest.mark.parametrize("variant", tg.VARIANTS)
def test_grid_inputs_tell_mistakes_from_the_truth(variant):
    """Every deliberate mistake moves jv on the GPU grid by at least 1e-2 relative (100x the GPU tolerance of 1e-4) in rel-L2
    and in rel-max on some case, and by at least 1e-3 (10x) on EVERY case it applies to.  Measured minimum / maximum over the
    cases, rel-L2: gn_drop_xhat_term 0.053 / 0.57, gn_gamma_first 0.0032 / 0.032 (the synthetic gammas are 1 +- 0.1),
    gelu_at_output 0.24 / 0.65, drop_skip 0.94 / 1.0, cond_drop_scale 0.125 / 0.134, row_map 0.47 / 1.0."""
    seen = []
    for case, K in tg.GRID:
        if not tg.applies(variant, case, K):
            continue
        r64, _ = tg.truth(case, K)
        wrong = tg.case_run(case, K, variant=variant)
        d2, dm = tr.rel_l2(wrong["jv"], r64["jv"]), tr.rel_max(wrong["jv"], r64["jv"])
        print(variant, tg.grid_id((case, K)), "rel-L2 %.3g rel-max %.3g" % (d2, dm))
        assert d2 >= 1e-3 and dm >= 1e-3, (variant, case, d2, dm)
        seen.append(min(d2, dm))
    assert seen and max(seen) >= 1e-2, (variant, seen)
    if variant == "row_map":
        assert any(B >= 2 and K >= 2 and B != K for (_, B, _, _, _), K in tg.GRID)


@pytest.mark.parametrize("g", tg.GRID, ids=tg.grid_id)
def test_float32_statement_is_well_conditioned(g):
    """The float32 run of the reference against its float64 run: measured 2.7e-7 .. 8.0e-7 rel-L2, 2.5e-7 .. 1.1e-6 rel-max, so
    the floor of the rule (1e-4) governs every case of the grid."""
    r64, r32 = tg.truth(*g)
    o2, om = tr.rel_l2(r32["jv"], r64["jv"]), tr.rel_max(r32["jv"], r64["jv"])
    print(tg.grid_id(g), "own rel-L2 %.3g rel-max %.3g" % (o2, om))
    assert 3 * o2 <= 1e-4 and 3 * om <= 1e-4, (o2, om)


# ---- ABI ------------------------------------------------------------------------------------------------------------------
def test_tangent_symbols_are_declared_exported_and_announced():
    from lns_amd import _lib
    _lib.build()
    src = open(os.path.join(ROOT, "include", "lns.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(lns_[a-z0-9_]+)\s*\(", code))
    L = _lib.lib()
    for s in SYMBOLS:
        assert s in declared and hasattr(L, s) and s in _lib.SYMBOLS, s
        assert getattr(L, s).argtypes is not None, s
    assert re.search(r"#define\s+LNS_ABI_VERSION\s+2\b", src)                      # additive: the version stays
    assert L.lns_build_has(b"rollout_tangent") == 1
    assert re.search(r"#define\s+LNS_TANGENT_MAX\s+%d\b" % _lib.LNS_TANGENT_MAX, src) and _lib.LNS_TANGENT_MAX == 32


@pytest.mark.parametrize("preset", ["ns2d_mini", "twophase_cond"])
def test_size_query_is_the_layout_formula_without_a_gpu(preset):
    """lns_train_workspace_bytes' layout under the current "train_wgrad" | 4 x [B*K, D, h, w] | [B*K, c, h, w], each part rounded
    up to 256 bytes; the existing size query keeps its value."""
    e = _engine(preset)
    L = e._L
    c, h, w = e.latent_shape()
    D = e.cfg.prop_n_embd
    nb = ctypes.c_size_t(0)
    seen = set()
    for form in (0, 1):
        e.set_option("train_wgrad", form)
        for B, T, K in ((1, 1, 1), (3, 2, 5), (2, 4, 32)):
            assert L.lns_train_workspace_bytes(e._h, B, h, w, T, ctypes.byref(nb)) == 0
            train = nb.value
            want = _round256(train) + 4 * _round256(4 * B * K * D * h * w) + _round256(4 * B * K * c * h * w)
            assert e.train_tangent_workspace_bytes(B, h, w, T, K) == want, (form, B, T, K)
            seen.add((B, T, train))
    assert len(seen) == 6          # the two forms size the training workspace differently, and the query follows


def test_refusal_matrix():
    """Code, message and order of every refusal of lns_train_tangent and its size query: null arguments, K, B * K, the step
    window, no propagator, then the devices (a fake pointer is not device memory: that is as far as a host gets), in
    include/lns.h's order -- of two failing checks the earlier one answers."""
    from lns_amd import _lib
    L = _lib.lib()
    e = _engine()
    ae_only = _engine(prop_kind=_lib.LNS_PROP_NONE)
    c, lh, lw = e.latent_shape()
    EINVAL, ESTATE = _lib.LNS_EINVAL, _lib.LNS_ESTATE

    def call(eng=e, params="own", B=2, T=4, K=3, t0=0, nsteps=4, v=P, jv=None, ws=P, nbytes=1 << 40):
        prm = _params(eng) if params == "own" else params
        rc = L.lns_train_tangent(eng._h, prm, B, lh, lw, T, K, t0, nsteps, v, jv, ws, nbytes, None)
        return rc, L.lns_last_error(eng._h).decode()
    assert L.lns_train_tangent(None, _params(e), 2, lh, lw, 4, 3, 0, 4, P, None, P, 1 << 40, None) == EINVAL
    matrix = [
        (dict(params=None), EINVAL, "tangent rollout: params array is null"),
        (dict(v=None), EINVAL, "tangent rollout: v is null"),
        (dict(params=None, K=0), EINVAL, "tangent rollout: params array is null"),
        (dict(K=0), EINVAL, "tangent rollout: K must be in 1 .. 32, got 0"),
        (dict(K=33), EINVAL, "tangent rollout: K must be in 1 .. 32, got 33"),
        (dict(K=-1, B=0, t0=-1), EINVAL, "tangent rollout: K must be in 1 .. 32, got -1"),
        (dict(B=0, t0=-1), EINVAL, "tangent rollout: B must be >= 1"),
        (dict(B=65535, K=2, nsteps=0), EINVAL, "tangent rollout: B * K = 131070 rows exceed the maximum of 65535 per call"),
        (dict(B=2048, K=32), EINVAL, "tangent rollout: B * K = 65536 rows exceed the maximum of 65535 per call"),
        (dict(t0=-1), EINVAL, "tangent rollout: steps t0 .. t0 + nsteps - 1 must lie in 0 .. T - 1 (T 4, t0 -1, nsteps 4)"),
        (dict(nsteps=0), EINVAL, "tangent rollout: steps t0 .. t0 + nsteps - 1 must lie in 0 .. T - 1 (T 4, t0 0, nsteps 0)"),
        (dict(t0=1, nsteps=4), EINVAL, "tangent rollout: steps t0 .. t0 + nsteps - 1 must lie in 0 .. T - 1 (T 4, t0 1, nsteps 4)"),
        (dict(T=0, nsteps=1), EINVAL, "tangent rollout: steps t0 .. t0 + nsteps - 1 must lie in 0 .. T - 1 (T 0, t0 0, nsteps 1)"),
        (dict(t0=2, nsteps=2147483647), EINVAL,
         "tangent rollout: steps t0 .. t0 + nsteps - 1 must lie in 0 .. T - 1 (T 4, t0 2, nsteps 2147483647)"),
        (dict(eng=ae_only, t0=5), EINVAL, "tangent rollout: steps t0 .. t0 + nsteps - 1 must lie in 0 .. T - 1 (T 4, t0 5, nsteps 4)"),
        (dict(eng=ae_only), ESTATE, "tangent rollout: engine has no propagator"),
        (dict(eng=ae_only, nbytes=0), ESTATE, "tangent rollout: engine has no propagator"),
        # the devices come before the workspace size: a short workspace behind a pointer that is no device memory
        (dict(nbytes=0), EINVAL, "training rollout: tensors must be HIP device memory"),
        (dict(ws=None), EINVAL, "training rollout: tensors must be HIP device memory"),
        (dict(), EINVAL, "training rollout: tensors must be HIP device memory"),
    ]
    for kw, want_rc, want_msg in matrix:
        rc, msg = call(**kw)
        assert rc == want_rc and msg == want_msg, (kw, rc, msg)
    # the size query: the same refusals in the same order, and nothing about devices
    nb = ctypes.c_size_t(0)

    def size(eng=e, B=2, T=4, K=3, out=nb):
        rc = L.lns_train_tangent_workspace_bytes(eng._h, B, lh, lw, T, K, ctypes.byref(out) if out is not None else None)
        return rc, L.lns_last_error(eng._h).decode()
    assert L.lns_train_tangent_workspace_bytes(None, 2, lh, lw, 4, 3, ctypes.byref(nb)) == EINVAL
    for kw, want_rc, want_msg in [
            (dict(out=None, K=0), EINVAL, "tangent rollout: bytes is null"),
            (dict(K=0, B=0), EINVAL, "tangent rollout: K must be in 1 .. 32, got 0"),
            (dict(K=33), EINVAL, "tangent rollout: K must be in 1 .. 32, got 33"),
            (dict(B=0, T=0), EINVAL, "tangent rollout: B must be >= 1"),
            (dict(B=4096, K=16, T=0), EINVAL, "tangent rollout: B * K = 65536 rows exceed the maximum of 65535 per call"),
            (dict(T=0, eng=ae_only), EINVAL, "tangent rollout: steps t0 .. t0 + nsteps - 1 must lie in 0 .. T - 1 (T 0, t0 0, nsteps 1)"),
            (dict(eng=ae_only), ESTATE, "tangent rollout: engine has no propagator")]:
        rc, msg = size(**kw)
        assert rc == want_rc and msg == want_msg, (kw, rc, msg)
    assert size()[0] == 0 and nb.value > 0


def test_orthonormalize_refuses_bad_arguments_without_a_device():
    from lns_amd import _lib
    L = _lib.lib()

    def call(v=P, B=2, K=3, n=32, r=None, logr=None):
        return L.lns_op_orthonormalize(v, B, K, n, r, logr, None), L.lns_create_error().decode()
    for kw, msg in [(dict(v=None, K=0), "orthonormalize: v is null"), (dict(K=0, n=0), "orthonormalize: K must be in 1 .. 32, got 0"),
                    (dict(K=33, B=0), "orthonormalize: K must be in 1 .. 32, got 33"), (dict(n=0, B=0), "orthonormalize: n must be >= 1"),
                    (dict(n=-5), "orthonormalize: n must be >= 1"), (dict(B=0), "orthonormalize: B must be >= 1"),
                    (dict(B=-1), "orthonormalize: B must be >= 1")]:
        assert call(**kw) == (_lib.LNS_EINVAL, msg), kw


def test_python_front_end_refuses_what_it_cannot_do():
    from lns_amd import config, dropin, engine, tangent
    from lns_amd._lib import LnsError
    with pytest.raises(LnsError, match="LatentDynamics"):
        tangent.TangentRollout(torch.nn.Linear(2, 2))
    m = dropin.build_dynamics(config.preset("ns2d_mini"))
    roll = tangent.TangentRollout(m)
    z = torch.zeros(1, 8, 4, 4)
    for kw, word in [(dict(T=0), "T >= 1"), (dict(T=4, renorm=0), "renorm >= 1"), (dict(T=4, burn_in=-1), "burn_in >= 0"),
                     (dict(T=4, k=0), "k must be in 1 .. 32"), (dict(T=4, k=33), "k must be in 1 .. 32"),
                     (dict(T=5, renorm=2), "positive multiple of renorm"), (dict(T=4, burn_in=4), "positive multiple of renorm"),
                     (dict(T=4, burn_in=1, renorm=2), "positive multiple of renorm"), (dict(T=4, chunk=0), "chunk"),
                     (dict(T=4, dt=0.0), "dt")]:
        with pytest.raises(LnsError, match=word):
            roll.lyapunov(z, **kw)
    with pytest.raises(LnsError, match="no CPU fallback"):          # every argument is fine: the model is not on a device
        roll.lyapunov(z, 4)
    with pytest.raises(LnsError, match="T must be >= 1"):
        roll.jvp(z, z, 0)
    with pytest.raises(LnsError, match="no CPU fallback"):
        roll.jvp(z, z, 2)
    with pytest.raises(LnsError, match="no CPU fallback"):
        engine.orthonormalize(torch.zeros(1, 2, 8))
    with pytest.raises(TypeError):
        m.lyapunov(z, 4, 0.5)                                        # a plain model takes no param


def test_new_kernels_use_no_scratch_and_spill_nothing():
    """tools/kernel_resources.py on the code object: the four new kernels have 0 scratch bytes and 0 spilled registers
    (memory-bound elementwise / reduction kernels: anything else would be a regression)."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    from lns_amd import _lib
    res = kernel_resources.resources(_lib.LIB_PATH)
    for name in ("gn_train_jvp_kernel", "gelu_jvp_kernel", "chan_scale_rows_kernel", "orthonormalize_kernel"):
        k = [v for n, v in res.items() if name in n]
        assert len(k) == 1, name
        assert k[0]["scratch"] == 0 and k[0]["vgpr_spill"] == 0 and k[0]["sgpr_spill"] == 0 and k[0]["vgpr"] <= 64, (name, k[0])

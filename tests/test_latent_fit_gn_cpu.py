"""CPU: the Gauss-Newton latent fit (include/lns.h "latent fit: Gauss-Newton").  The six calls are declared, exported and
announced and refuse bad arguments before any device work (fake pointers, no GPU here); the size queries equal their
documented parts; the float64 statement (tests/latent_fit_gn_reference.py) is the operator assembled from an explicit
Jacobian, symmetric, with v^T H v the tangent-side formula; conjugate gradients on it converge; a frozen sample keeps its bits;
four deliberate mistakes are told from the statement; the twin experiments reach the recorded factors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import latent_fit_gn_reference as gn
import latent_fit_reference as lf
import train_reference as tr
from helpers import ROOT

GN_SYMBOLS = ("lns_train_gn_product_workspace_bytes", "lns_train_gn_product", "lns_op_cg_start", "lns_op_cg_update",
              "lns_fit_gn_step_workspace_bytes", "lns_fit_gn_step")
P = ctypes.c_void_p(0x1000)
Q = ctypes.c_void_p(0x2000)


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


def test_gn_symbols_are_declared_exported_and_announced():
    from lns_amd import _lib
    _lib.build()
    src = open(os.path.join(ROOT, "include", "lns.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(lns_[a-z0-9_]+)\s*\(", code))
    L = _lib.lib()
    for s in GN_SYMBOLS:
        assert s in declared and hasattr(L, s) and s in _lib.SYMBOLS, s
    assert re.search(r"#define\s+LNS_ABI_VERSION\s+2\b", src)                      # additive: the version stays
    assert L.lns_build_has(b"fit_gauss_newton") == 1
    assert ctypes.sizeof(_lib.LnsGnSpec) == 56
    assert re.search(r"#define\s+LNS_GN_CG_MAX\s+%d\b" % _lib.LNS_GN_CG_MAX, src)


def test_cg_ops_refuse_bad_arguments_without_a_device():
    from lns_amd import _lib
    L = _lib.lib()

    def cerr():
        return L.lns_create_error().decode()

    def start(g=P, x=P, r=P, p=P, B=2, n=33, rs=P, rs0=P):
        return L.lns_op_cg_start(g, x, r, p, B, n, rs, rs0, None)

    def update(x=P, r=P, p=P, hp=P, php=None, B=2, n=33, tol=0.0, rs=P, rs0=P, applied=None):
        return L.lns_op_cg_update(x, r, p, hp, php, B, n, tol, rs, rs0, applied, None)
    for kw, word in ((dict(g=None), "g"), (dict(x=None), "x"), (dict(r=None), "r"), (dict(p=None), "p"), (dict(rs=None), "rs"),
                     (dict(rs0=None), "rs0"), (dict(B=0), "B"), (dict(B=65536), "B"), (dict(n=0), "n"), (dict(n=1 << 31), "n")):
        assert start(**kw) == _lib.LNS_EINVAL, kw
        assert cerr().startswith("cg start") and word in cerr(), (kw, cerr())
    for kw, word in ((dict(x=None), "x"), (dict(r=None), "r"), (dict(p=None), "p"), (dict(hp=None), "hp"), (dict(rs=None), "rs"),
                     (dict(rs0=None), "rs0"), (dict(B=0), "B"), (dict(n=0), "n"), (dict(tol=-1e-3), "tol"),
                     (dict(tol=float("nan")), "tol"), (dict(tol=float("inf")), "tol")):
        assert update(**kw) == _lib.LNS_EINVAL, kw
        assert cerr().startswith("cg update") and word in cerr(), (kw, cerr())


def test_gn_product_and_step_refuse_bad_arguments_without_a_device():
    from lns_amd import _lib, engine
    L = _lib.lib()
    e = _engine()
    h = e._h
    c, lh, lw = e.latent_shape()
    prm = _params(e)

    def err(eng=h):
        return L.lns_last_error(eng).decode()

    def arrays(steps, weights):
        st = (ctypes.c_int * max(1, len(steps)))(*steps) if steps is not None else None
        w = (ctypes.c_double * max(1, len(weights)))(*weights) if weights is not None else None
        return st, w

    # ---- lns_train_gn_product ----
    def prod(eng=h, params=prm, z_in=P, z_pred=P, B=3, T=3, steps=(0, 2), weights=(1.0, 0.5), lam=0.0, mu=0.0, v=P, hv=Q, vhv=None, ws=P,
             nbytes=1 << 40, hh=lh, ww=lw):
        st, w = arrays(steps, weights)
        return L.lns_train_gn_product(eng, params, z_in, z_pred, B, hh, ww, T, len(steps) if steps is not None else 1, st, w, lam, mu, v,
                                      hv, vhv, ws, nbytes, None)
    assert prod(eng=None) == _lib.LNS_EINVAL
    cases = [(dict(params=None), "params"), (dict(z_in=None), "z_in"), (dict(z_pred=None), "z_pred"), (dict(v=None), "v"),
             (dict(hv=None), "hv"), (dict(hv=P), "must not be v"), (dict(B=0), "B"), (dict(hh=0), "latent size"),
             (dict(steps=(), weights=()), "n_obs"), (dict(steps=tuple(range(65)), weights=(1.0,) * 65, T=65), "n_obs"),
             (dict(steps=None), "obs_steps"), (dict(steps=(2, 0)), "ascending"), (dict(steps=(0, 0)), "ascending"),
             (dict(steps=(-1, 2)), "ascending"), (dict(weights=(1.0, -1.0)), "obs_weight"), (dict(weights=(float("nan"), 1.0)), "obs_weight"),
             (dict(lam=-0.5), "background"), (dict(lam=float("inf")), "background"),
             (dict(T=4), "last observed step + 1"), (dict(T=2), "last observed step + 1"), (dict(steps=(0, 3)), "last observed step + 1"),
             (dict(mu=-1.0), "damping"), (dict(mu=float("nan")), "damping")]
    for kw, word in cases:
        assert prod(**kw) == _lib.LNS_EINVAL, kw
        assert word in err(), (kw, err())
    # the documented order: the observation table before T, T before the damping, the damping before the workspace
    assert prod(steps=(2, 0), T=7, mu=-1.0, nbytes=0) == _lib.LNS_EINVAL and "ascending" in err()
    assert prod(T=7, mu=-1.0, nbytes=0) == _lib.LNS_EINVAL and "last observed step" in err()
    assert prod(mu=-1.0, nbytes=0) == _lib.LNS_EINVAL and "damping" in err()
    first = next(i for i, (k, _, isb) in enumerate(e.params) if k.startswith("propagator.") and not isb)
    broken = _params(e)
    broken[first] = None
    assert prod(params=broken, nbytes=0) == _lib.LNS_EINVAL and e.params[first][0] in err()
    # the workspace: the documented layout, and a short one is refused with the needed size in the message
    n = c * lh * lw
    need = e.train_gn_product_workspace_bytes(3, lh, lw, 3, 2)
    assert need == e.train_tangent_workspace_bytes(3, lh, lw, 3, 1) + _round256(4 * 3 * 3 * n) + _round256(8 * 3 * 3)
    assert prod(nbytes=need - 1) == _lib.LNS_ENOMEM and "workspace" in err() and str(need) in err()
    assert prod(ws=None) == _lib.LNS_ENOMEM
    nb = ctypes.c_size_t(0)
    for fn in (L.lns_train_gn_product_workspace_bytes, L.lns_fit_gn_step_workspace_bytes):
        for args in ((0, lh, lw, 3, 2), (3, lh, lw, 0, 2), (3, lh, lw, 3, 0), (3, lh, lw, 3, 65), (3, 0, lw, 3, 2)):
            assert fn(h, *args, ctypes.byref(nb)) == _lib.LNS_EINVAL, args
        assert fn(h, 3, lh, lw, 3, 2, None) == _lib.LNS_EINVAL
    for B, T, n_obs in ((1, 1, 1), (33, 5, 64), (5, 2, 2)):
        prod_need = e.train_gn_product_workspace_bytes(B, lh, lw, T, n_obs)
        assert prod_need == e.train_tangent_workspace_bytes(B, lh, lw, T, 1) + _round256(4 * B * T * n) + _round256(8 * B * (n_obs + 1))
        assert e.fit_gn_step_workspace_bytes(B, lh, lw, T, n_obs) == prod_need + _round256(4 * B * T * n) + 6 * _round256(4 * B * n) \
            + 3 * _round256(8 * B)

    # ---- lns_fit_gn_step ----
    def spec_of(steps=(0, 2), weights=(1.0, 0.5), lam=0.0, n_cg=8, mu=0.0, tol=0.0, **kw):
        s = engine.gn_spec(steps, weights, lam, n_cg=n_cg, damping=mu, cg_tol=tol)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def raw_spec(steps, weights):
        """a spec whose table gn_spec itself would refuse"""
        s = spec_of()
        s._steps, s._weights = arrays(steps, weights)
        s.obs_steps = ctypes.cast(s._steps, ctypes.POINTER(ctypes.c_int))
        s.obs_weight = ctypes.cast(s._weights, ctypes.POINTER(ctypes.c_double))
        s.n_obs = len(steps)
        return s

    def step(eng=h, params=prm, z0=P, param=None, obs=P, zb=None, B=3, spec=None, loss=P, ws=P, nbytes=1 << 40, hh=lh, ww=lw):
        spec = spec_of() if spec is None else spec
        return L.lns_fit_gn_step(eng, params, z0, param, obs, zb, B, hh, ww, ctypes.byref(spec) if spec != "null" else None, loss, None,
                                 None, None, ws, nbytes, None)
    assert step(eng=None) == _lib.LNS_EINVAL
    cases = [(dict(spec="null"), "spec"), (dict(spec=spec_of(size=48)), "size"), (dict(spec=spec_of(flags=1)), "flags"),
             (dict(spec=spec_of(n_cg=0)), "n_cg"), (dict(spec=spec_of(n_cg=65)), "n_cg"), (dict(spec=spec_of(n_cg=-3)), "n_cg"),
             (dict(spec=spec_of(tol=-1e-3)), "cg_tol"), (dict(spec=spec_of(tol=float("nan"))), "cg_tol"),
             (dict(params=None), "params"), (dict(z0=None), "z0"), (dict(obs=None), "obs"), (dict(loss=None), "loss"),
             (dict(spec=spec_of(lam=0.5)), "z_background"), (dict(B=0), "B"),
             (dict(spec=raw_spec((2, 0), (1.0, 1.0))), "ascending"), (dict(spec=raw_spec((0, 1 << 24), (1.0, 1.0))), "ascending"),
             (dict(spec=raw_spec((0, 2), (1.0, -1.0))), "obs_weight"), (dict(spec=raw_spec((), ())), "n_obs"),
             (dict(spec=raw_spec(tuple(range(65)), (1.0,) * 65)), "n_obs"), (dict(spec=spec_of(lam=-0.5), zb=P), "background"),
             (dict(spec=spec_of(mu=-1.0)), "damping"), (dict(spec=spec_of(mu=float("inf"))), "damping")]
    for kw, word in cases:
        assert step(**kw) == _lib.LNS_EINVAL, kw
        assert err().startswith("gn step") or err().startswith("obs loss"), err()
        assert word in err(), (kw, err())
    # the documented order: the spec's own fields before the pointers, the pointers before the table, the table before the workspace
    assert step(spec=spec_of(n_cg=0), params=None) == _lib.LNS_EINVAL and "n_cg" in err()
    assert step(params=None, spec=raw_spec((2, 0), (1.0, 1.0))) == _lib.LNS_EINVAL and "params" in err()
    assert step(spec=spec_of(mu=-1.0), nbytes=0) == _lib.LNS_EINVAL and "damping" in err()
    assert step(params=broken, nbytes=0) == _lib.LNS_EINVAL and e.params[first][0] in err()
    need = e.fit_gn_step_workspace_bytes(3, lh, lw, 3, 2)
    assert step(nbytes=need - 1) == _lib.LNS_ENOMEM and "workspace" in err() and str(need) in err()
    assert step(ws=None) == _lib.LNS_ENOMEM
    # an engine without a propagator
    ae_only = _engine(prop_kind=_lib.LNS_PROP_NONE)
    assert step(eng=ae_only._h, params=_params(ae_only)) == _lib.LNS_ESTATE and "propagator" in err(ae_only._h)
    assert prod(eng=ae_only._h, params=_params(ae_only)) == _lib.LNS_ESTATE and "propagator" in err(ae_only._h)
    assert L.lns_fit_gn_step_workspace_bytes(ae_only._h, 3, lh, lw, 3, 2, ctypes.byref(nb)) == _lib.LNS_ESTATE
    assert L.lns_train_gn_product_workspace_bytes(ae_only._h, 3, lh, lw, 3, 2, ctypes.byref(nb)) == _lib.LNS_ESTATE
    # the conditional propagator: param is required (and is all that differs)
    ce = _engine("twophase_cond")
    _, ch, cw = ce.latent_shape()
    assert step(eng=ce._h, params=_params(ce), hh=ch, ww=cw) == _lib.LNS_EINVAL and "param" in err(ce._h)
    assert step(eng=ce._h, params=_params(ce), hh=ch, ww=cw, param=P, nbytes=16) == _lib.LNS_ENOMEM


def test_python_front_end_refuses_what_it_cannot_do():
    from lns_amd import config, dropin, engine, fit
    from lns_amd._lib import LnsError
    with pytest.raises(LnsError):
        engine.gn_spec((2, 1))
    assert engine.gn_spec((0, 2), n_cg=5, damping=0.25).n_cg == 5
    m = dropin.build_dynamics(config.preset("ns2d_mini"))
    with pytest.raises(LnsError, match="no CPU fallback"):
        fit.LatentFit(m).run_gauss_newton(torch.zeros(1, 8, 4, 4), torch.zeros(1, 1, 8, 4, 4), [0])
    with pytest.raises(LnsError, match="no CPU fallback"):
        engine.cg_start(torch.zeros(1, 4), torch.zeros(1, 4), torch.zeros(1, 4), torch.zeros(1, 4))
    cargs = tr.engine_args("E6")
    cm = dropin.build_dynamics(cargs)
    assert fit.LatentFit(cm).fit_param is True                       # fit_param=None on a conditional model: not a refusal here
    with pytest.raises(LnsError, match="no param direction"):
        fit.LatentFit(cm, fit_param=True).run_gauss_newton(torch.zeros(1, 8, 4, 4), torch.zeros(1, 1, 8, 4, 4), [0], param=torch.zeros(1))
    x = torch.zeros(1, cargs.in_channels, cargs.Ly, cargs.Lx)
    with pytest.raises(LnsError, match="no param direction"):
        cm.assimilate(x, x[:, None], [0], torch.zeros(1), method="gauss_newton", fit_param=True)
    with pytest.raises(LnsError, match="method"):
        cm.assimilate(x, x[:, None], [0], torch.zeros(1), method="newton")


# ---- the float64 statement -----------------------------------------------------------------------------------------------
SMALL = ("E5", 1, 2, 2, 2)                    # n = 32: the Jacobian is a 32 x 32 matrix per step


def _small(lam=gn.GN_LAMBDA, mu=gn.GN_DAMPING):
    z0, prm, v, u = gn.case_start(SMALL)
    steps, w = gn.case_obs(SMALL)
    prop = lf.propagator(SMALL[0])
    t = lambda a: torch.from_numpy(a).double() if a is not None else None      # noqa: E731
    return prop, t(z0), t(prm), t(v), t(u), steps, w


@pytest.mark.parametrize("lam,mu", [(0.0, 0.0), (gn.GN_LAMBDA, gn.GN_DAMPING)])
def test_product_is_the_matrix_of_the_explicit_jacobian(lam, mu):
    prop, z0, prm, v, u, steps, w = _small()
    H = gn.gn_matrix(prop, z0, prm, steps, w, lam, mu)
    with torch.no_grad():
        hv, vhv, jv = gn.gn_product(prop, z0, prm, v, steps, w, lam, mu)
        hu, uhu, _ = gn.gn_product(prop, z0, prm, u, steps, w, lam, mu)
    B, n = z0.shape[0], z0[0].numel()
    ref = torch.einsum("bij,bj->bi", H, v.reshape(B, n))
    assert tr.rel_max(hv.reshape(B, n).numpy(), ref.numpy()) <= 1e-12
    assert tr.rel_max(H.numpy(), H.transpose(1, 2).numpy()) <= 1e-13                         # H is symmetric
    uHv, vHu = (u * hv).reshape(B, -1).sum(1), (v * hu).reshape(B, -1).sum(1)
    assert torch.allclose(uHv, vHu, rtol=1e-12, atol=0)
    # v^T H v from the tangent side alone is <v, H v>, and not negative
    assert torch.allclose(vhv, (v * hv).reshape(B, -1).sum(1), rtol=1e-12, atol=0) and (vhv >= 0).all() and (uhu >= 0).all()
    cw = [2.0 * wk / n for wk in w]
    tangent_side = sum(cw[k] * (jv[:, k] ** 2).reshape(B, -1).sum(1) for k in range(len(steps))) + (2 * lam / n + mu) * (v ** 2).reshape(B, -1).sum(1)
    assert torch.allclose(vhv, tangent_side, rtol=1e-14, atol=0)


def test_float64_cg_converges_within_n_steps():
    """|r| / |g| <= 1e-10 after at most n = 32 steps on the damped operator (H = J^T W J + (2 lambda / n + mu) I)."""
    prop, z0, prm, v, u, steps, w = _small()
    n = z0[0].numel()
    with torch.no_grad():
        delta, resid = gn.cg_solve(lambda p: gn.gn_product(prop, z0, prm, p, steps, w, gn.GN_LAMBDA, gn.GN_DAMPING)[:2], v, n)
        hd, _, _ = gn.gn_product(prop, z0, prm, delta, steps, w, gn.GN_LAMBDA, gn.GN_DAMPING)
    print("CG residual after %d steps" % n, resid.numpy())
    assert (resid <= 1e-10).all(), resid
    assert float((hd + v).norm() / v.norm()) <= 1e-9                                         # H delta = -g


def test_order_exact_statement_solves_and_freezes():
    """The numpy statement of lns_op_cg_start / lns_op_cg_update on an explicit SPD matrix: it converges to float32 level, php
    given equals php computed when the caller sums in the same order, and a frozen sample (g = 0, php = 0, php = NaN, or the
    tolerance reached) keeps every bit."""
    rng = np.random.RandomState(3)
    B, n = 3, 257
    A = rng.randn(B, n, n)
    H = np.einsum("bij,bkj->bik", A, A) / n + 0.5 * np.eye(n)[None]
    g = rng.randn(B, n).astype(np.float32)
    g[1] = 0                                                                                  # a frozen sample among active ones
    mv = lambda p: np.einsum("bij,bj->bi", H, p.astype(np.float64)).astype(np.float32)        # noqa: E731
    x, r, p, rs, rs0 = gn.cg_start(g)
    assert (x == 0).all() and np.array_equal(r, -g) and np.array_equal(p, r) and rs[1] == 0 and np.array_equal(rs, rs0)
    applied = None
    # eigenvalues of H lie in about (0.5, 4.5): kappa ~ 9, CG's bound 2 ((sqrt(kappa) - 1) / (sqrt(kappa) + 1))^k = 2 * 0.5^k is
    # 1.2e-7 at k = 24, below float32's floor; 1e-4 is asked
    for _ in range(24):
        hp = mv(p)
        php = np.array([gn.block_sum(p[b].astype(np.float64) * hp[b].astype(np.float64)) for b in range(B)])
        a = gn.cg_update(x, r, p, hp, rs, rs0, php=php, applied=applied)
        b_ = gn.cg_update(x, r, p, hp, rs, rs0, applied=applied)
        for s, t in zip(a, b_):
            assert np.array_equal(s, t)
        x, r, p, rs, applied = a
    assert (applied == [24, 0, 24]).all() and (x[1] == 0).all() and (r[1] == 0).all() and rs[1] == 0
    assert (np.sqrt(rs[[0, 2]] / rs0[[0, 2]]) <= 1e-4).all(), np.sqrt(rs / rs0)
    # frozen by php = 0, php = NaN, php < 0 and by the tolerance: every array keeps its bits
    hp = mv(p)
    for php, tol in ((np.zeros(B), 0.0), (np.full(B, np.nan), 0.0), (np.full(B, -1.0), 0.0), (np.ones(B), 1.0)):
        out = gn.cg_update(x, r, p, hp, rs, rs0, php=php, tol=tol, applied=applied)
        for s, t in zip(out, (x, r, p, rs, applied)):
            assert np.array_equal(s, t)
        assert np.isfinite(out[0]).all()


def test_block_sum_is_the_documented_order():
    """Against a lane-by-lane loop written the slow way, at sizes below, at and above a block and a wave."""
    rng = np.random.RandomState(0)
    for n in (1, 63, 64, 255, 256, 257, 1040):
        t = rng.randn(n) * 10.0 ** rng.randint(-3, 4, n)
        acc = [0.0] * 256
        for i in range(n):
            acc[i % 256] = acc[i % 256] + t[i]
        waves = []
        for wv in range(4):
            v = acc[64 * wv:64 * wv + 64]
            for m in (1, 2, 4, 8, 16, 32):
                v = [v[l] + v[l ^ m] for l in range(64)]
            waves.append(v[0])
        assert gn.block_sum(t) == (waves[0] + waves[1]) + (waves[2] + waves[3]), n


@pytest.mark.parametrize("mistake", gn.MISTAKES)
def test_deliberate_mistakes_are_told_from_the_statement(mistake):
    """Each mistake moves the result by far more than the GPU tests' tolerance (1e-4) on the inputs they use."""
    case = ("E6", 5, 2, 7, 15)
    z0, prm, v, u = gn.case_start(case)
    steps, w = gn.case_obs(case)
    prop = lf.propagator(case[0])
    t = lambda a: torch.from_numpy(a).double() if a is not None else None      # noqa: E731
    lam, mu = gn.GN_LAMBDA, gn.GN_DAMPING
    with torch.no_grad():
        good = gn.gn_product(prop, t(z0), t(prm), t(v), steps, w, lam, mu)
        if mistake != "beta_inverted":
            bad = gn.gn_product(prop, t(z0), t(prm), t(v), steps, w, lam, mu, mistake=mistake)
            d_hv, d_vhv = tr.rel_l2(bad[0].numpy(), good[0].numpy()), tr.rel_max(bad[1].numpy(), good[1].numpy())
            print(mistake, "moves hv by %.3g, vhv by %.3g" % (d_hv, d_vhv))
            assert d_hv >= 1e-2 and d_vhv >= 1e-2, (d_hv, d_vhv)
            return
        mv = lambda p: gn.gn_product(prop, t(z0), t(prm), p, steps, w, lam, mu)[:2]      # noqa: E731
        x_good, r_good = gn.cg_solve(mv, t(v), 4)
        x_bad, r_bad = gn.cg_solve(mv, t(v), 4, mistake=mistake)
    d = tr.rel_l2(x_bad.numpy(), x_good.numpy())
    print(mistake, "moves the CG iterate by %.3g; residuals %s against %s" % (d, r_bad.numpy(), r_good.numpy()))
    assert d >= 1e-2, d
    # and in the order-exact statement: the direction after one step differs
    g = v.reshape(v.shape[0], -1)
    x, r, p, rs, rs0 = gn.cg_start(g)
    hp = (0.5 * p).astype(np.float32)
    a, b = gn.cg_update(x, r, p, hp, rs, rs0), gn.cg_update(x, r, p, hp, rs, rs0, mistake=mistake)
    assert np.array_equal(a[0], b[0]) and not np.array_equal(a[2], b[2])


@pytest.mark.parametrize("setup", lf.TWINS, ids=tr.case_id)
def test_reference_gauss_newton_reaches_the_recorded_factors(setup):
    """Float64, param known, observations at steps [0, 2] with weights [1, 0.5], no damping, no line search.  Measured with this
    reference, worst sample of loss[0] / loss[-1] (latent_fit_gn_reference.MEASURED):
        1 outer x 8 CG     E6 7x15 17.5x     E6 2x2 9.2x     E3 4x4 17.2x
        3 outer x 8 CG     E6 7x15 341x      E6 2x2 982x     E3 4x4 550x
    asserted at 0.6 of the measured value; every loss sequence is monotone; the state error against the truth falls to
    0.36 - 0.54 of the start's (asserted: below 0.7)."""
    d = lf.twin(setup)
    for outer in (1, 3):
        z, loss = gn.twin_fit(setup, outer=outer)
        l = loss.numpy()
        red = l[0] / l[-1]
        print(tr.case_id(setup), "%d x %d: loss reduction" % (outer, gn.CG_ITERS), red)
        assert (red >= gn.CPU_FRACTION * gn.MEASURED[(outer, gn.CG_ITERS)][setup]).all(), red
        assert (red.min() <= gn.MEASURED[(outer, gn.CG_ITERS)][setup] / gn.CPU_FRACTION), red      # the record is not stale
        assert (np.diff(l, axis=0) <= 0).all(), l
    B = setup[1]
    e0 = np.sqrt(((d["z_start"].astype(np.float64) - d["z_true"]) ** 2).reshape(B, -1).sum(1))
    e1 = np.sqrt(((z.numpy() - d["z_true"]) ** 2).reshape(B, -1).sum(1))
    print(tr.case_id(setup), "state error / start's", e1 / e0)
    assert (e1 / e0 <= 0.7).all(), e1 / e0


def test_new_kernels_use_no_scratch_and_spill_nothing():
    """tools/kernel_resources.py on the code object: the Gauss-Newton kernels have 0 scratch bytes and 0 spilled registers
    (memory-bound elementwise / reduction kernels: anything else would be a regression)."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    from lns_amd import _lib
    res = kernel_resources.resources(_lib.LIB_PATH)
    for name in ("gn_weight_kernel", "gn_vhv_kernel", "gn_axpy_kernel", "cg_start_kernel", "cg_update_kernel", "cg_resid_kernel"):
        k = [v for n, v in res.items() if name in n]
        assert len(k) == 1, name
        assert k[0]["scratch"] == 0 and k[0]["vgpr_spill"] == 0 and k[0]["sgpr_spill"] == 0 and k[0]["vgpr"] <= 64, (name, k[0])

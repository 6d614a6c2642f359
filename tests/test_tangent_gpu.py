"""GPU: lns_train_tangent, lns_op_orthonormalize and the Lyapunov loop built on them.

  * jv at every stored step against forward-mode autograd in float64 (tests/tangent_reference.py) within
    latent_fit_reference.rule -- max(1e-4, 3 x the float32 statement's own error) in rel-L2 and in rel-max -- on the grid of
    tangent_reference.GRID under both "train_wgrad" values (the workspace layout differs);
  * <J v, w> = <v, J^T w> between lns_train_tangent and the state-only lns_train_backward_ex, ours against ours;
  * structure: a split call, jv_out's last step, a repeated call (bits); one (sample, tangent) alone (the rule);
  * lns_op_orthonormalize: Q R reconstructs the input, Q and log R_kk against the float64 statement, |Q^T Q - I| against
    the fp32 statement, a zero vector, accumulation, an unaligned pointer;
  * TangentRollout.lyapunov against the float64 loop from the same start vectors; chunking and burn_in (bits);
    LatentDynamics.lyapunov end to end."""
import numpy as np
import pytest
import torch

import latent_fit_reference as lf
import tangent_reference as tg
import train_reference as tr

pytestmark = pytest.mark.gpu


def _need_gpu():
    assert torch.cuda.is_available(), "GPU test selected but no GPU is visible"


def test_rollout_tangent_is_built():
    """Fails on the parent: the symbols and the feature name."""
    from lns_amd import _lib
    L = _lib.lib()
    for s in ("lns_train_tangent_workspace_bytes", "lns_train_tangent", "lns_op_orthonormalize"):
        assert hasattr(L, s), s
    assert L.lns_build_has(b"rollout_tangent") == 1


def _setup(case, K, form=0):
    """model, engine, params, z0, param, v, z_pred, the shared workspace -- after the training forward."""
    name, B, T, h, w = case
    model = tr.grid_model(name)
    eng = model._owner._eng
    eng.set_option("train_wgrad", form)
    z0, prm, v = tg.case_start(case, K)
    params = {k: p.detach() for k, p in model.named_parameters() if k.startswith("propagator.")}
    z0 = torch.from_numpy(z0).cuda()
    p = torch.from_numpy(prm).cuda() if prm is not None else None
    v = torch.from_numpy(v).cuda()
    ws = torch.empty(eng.train_tangent_workspace_bytes(B, h, w, T, K), dtype=torch.uint8, device="cuda")
    z_pred, _ = eng.train_forward(params, z0, T, param=p, workspace=ws)
    return model, eng, params, z0, p, v, z_pred, ws


def _tangent(eng, params, v, T, ws, **kw):
    vv = v.clone()
    jv = eng.train_tangent(params, vv, T, ws, keep=True, **kw)
    return vv, jv


# ---- parity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", tr.FORMS)
@pytest.mark.parametrize("g", tg.GRID, ids=tg.grid_id)
def test_jv_against_float64(g, form):
    _need_gpu()
    case, K = g
    name, B, T, h, w = case
    model, eng, params, z0, p, v, z_pred, ws = _setup(case, K, form)
    vv, jv = _tangent(eng, params, v, T, ws)
    torch.cuda.synchronize()
    assert jv.shape == (B, K, T) + tuple(z0.shape[1:])
    # the forward on the larger workspace is the forward: the existing call keeps its bits
    z_plain, _ = eng.train_forward(params, z0, T, param=p)
    assert torch.equal(z_plain, z_pred)
    r64, r32 = tg.truth(case, K)
    ours = jv.cpu().numpy()
    assert np.isfinite(ours).all()
    for s in range(T):
        e2, b2, em, bm, o2, om = lf.rule(ours[:, :, s], r64["jv"][:, :, s], r32["jv"][:, :, s])
        print("%s form %d step %d: rel-L2 %.2e/%.2e rel-max %.2e/%.2e (own %.2e %.2e)" % (tg.grid_id(g), form, s, e2, b2, em, bm, o2, om))
        assert e2 <= b2, ("rel-L2", s, e2, b2, o2)
        assert em <= bm, ("rel-max", s, em, bm, om)


@pytest.mark.parametrize("g", tg.DOT_GRID, ids=tg.grid_id)
def test_tangent_pairs_with_the_adjoint(g):
    """|<J v, w> - <v, J^T w>| <= 2e-4 |J v| |w| per (sample, tangent): each side is held to 1e-4 of the truth."""
    _need_gpu()
    from lns_amd import filler
    case, K = g
    name, B, T, h, w = case
    model, eng, params, z0, p, v, z_pred, ws = _setup(case, K)
    vv, jv = _tangent(eng, params, v, T, ws)
    wv = torch.from_numpy(filler.normal("tangent_w", tuple(z0.shape), 5)).cuda()
    g_pred = torch.zeros_like(z_pred)
    g_pred[:, -1] = wv
    _, gz = eng.train_backward(params, z0, z_pred, g_pred, ws, need_z_grad=True, state_only=True)
    torch.cuda.synchronize()
    jl, w64, v64, g64 = (t.double().cpu() for t in (jv[:, :, -1], wv, v, gz))
    for k in range(K):
        lhs = (jl[:, k] * w64).reshape(B, -1).sum(1)
        rhs = (v64[:, k] * g64).reshape(B, -1).sum(1)
        scale = jl[:, k].reshape(B, -1).norm(dim=1) * w64.reshape(B, -1).norm(dim=1)
        rel = ((lhs - rhs).abs() / scale).max().item()
        print(tg.grid_id(g), "k", k, "dot-product defect %.3g" % rel)
        assert rel <= 2e-4, (k, rel)


# ---- structure ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", [(("E3", 4, 5, 8, 8), 3), (("E6", 5, 2, 7, 15), 3)], ids=tg.grid_id)
def test_split_last_step_and_repeat_are_bitwise(g):
    _need_gpu()
    from lns_amd import _lib
    case, K = g
    name, B, T, h, w = case
    model, eng, params, z0, p, v, z_pred, ws = _setup(case, K)
    v_all, jv_all = _tangent(eng, params, v, T, ws)
    assert torch.equal(jv_all[:, :, -1], v_all)                       # jv_out's last step is v after the call
    v_again, jv_again = _tangent(eng, params, v, T, ws)
    assert torch.equal(jv_again, jv_all) and torch.equal(v_again, v_all)
    for s in range(1, T):
        vs = v.clone()
        a = eng.train_tangent(params, vs, T, ws, t0=0, nsteps=s, keep=True)
        assert torch.equal(vs, jv_all[:, :, s - 1])
        b = eng.train_tangent(params, vs, T, ws, t0=s, nsteps=T - s, keep=True)
        assert torch.equal(torch.cat([a, b], 2), jv_all) and torch.equal(vs, v_all), s
    v_none = v.clone()
    assert eng.train_tangent(params, v_none, T, ws) is None and torch.equal(v_none, v_all)       # without jv_out: the same v
    # the workspace check (the last refusal: it needs real device pointers to be reached)
    need = eng.train_tangent_workspace_bytes(B, h, w, T, K)
    rc = eng._L.lns_train_tangent(eng._h, eng._ptr_array(params), B, h, w, T, K, 0, T, v_none.data_ptr(), None, ws.data_ptr(), need - 1,
                                  eng._stream(v))
    assert rc == _lib.LNS_ENOMEM and str(need) in eng._L.lns_last_error(eng._h).decode()
    torch.cuda.synchronize()
    assert torch.equal(v_none, v_all)                                  # a refused call touches nothing


@pytest.mark.parametrize("g", [(("E3", 4, 5, 8, 8), 3), (("E6", 5, 2, 7, 15), 3)], ids=tg.grid_id)
def test_one_tangent_alone_agrees_with_its_row(g):
    """B = 1, K = 1 against row (b, k) of the batch, under the rule (the plan's tiling may differ with B*K: no bits promised)."""
    _need_gpu()
    case, K = g
    name, B, T, h, w = case
    model, eng, params, z0, p, v, z_pred, ws = _setup(case, K)
    b, k = B - 1, K - 1
    ws1 = torch.empty(eng.train_tangent_workspace_bytes(1, h, w, T, 1), dtype=torch.uint8, device="cuda")
    eng.train_forward(params, z0[b:b + 1], T, param=p[b:b + 1] if p is not None else None, workspace=ws1)
    _, jv1 = _tangent(eng, params, v[b:b + 1, k:k + 1].contiguous(), T, ws1)
    torch.cuda.synchronize()
    r64, r32 = tg.truth(case, K)
    e2, b2, em, bm, o2, om = lf.rule(jv1[0, 0].cpu().numpy(), r64["jv"][b, k], r32["jv"][b, k])
    print(tg.grid_id(g), "alone: rel-L2 %.2e/%.2e rel-max %.2e/%.2e" % (e2, b2, em, bm))
    assert e2 <= b2 and em <= bm, (e2, b2, em, bm)


# ---- orthonormalisation -----------------------------------------------------------------------------------------------------
ORTH_TOL = 2e-7


def _orth(v_np, offset=False):
    """(Q, R, log R_kk) of the HIP op, numpy float64; offset: the vectors start one float past an aligned allocation."""
    from lns_amd import engine
    B, K, n = v_np.shape
    if offset:
        buf = torch.empty(B * K * n + 1, dtype=torch.float32, device="cuda")
        v = buf[1:].view(B, K, n)
        assert v.data_ptr() % 8 == 4 and v.is_contiguous()
        v.copy_(torch.from_numpy(v_np))
    else:
        v = torch.from_numpy(v_np).cuda()
    logr = torch.zeros((B, K), dtype=torch.float64, device="cuda")
    q, r = engine.orthonormalize(v, need_r=True, logr_acc=logr)
    torch.cuda.synchronize()
    assert q.data_ptr() == v.data_ptr()
    return q.double().cpu().numpy(), r.cpu().numpy(), logr.cpu().numpy()


def _reconstruct(Q, R):
    return np.einsum("bjk,bjn->bkn", np.asarray(R, np.float64), np.asarray(Q, np.float64))


def _gram_defect(Q):
    Q = np.asarray(Q, np.float64)
    return float(np.abs(np.einsum("bjn,bkn->bjk", Q, Q) - np.eye(Q.shape[1])[None]).max())


@pytest.mark.parametrize("family", ["normal", "tiny", "huge"])
@pytest.mark.parametrize("shape", tg.ORTH_SHAPES + ["offset"], ids=str)
def test_orthonormalize(shape, family):
    _need_gpu()
    offset = shape == "offset"
    shape = (3, 4, 257) if offset else shape
    v = tg.orth_input(shape, family)
    Q, R, logr = _orth(v, offset)
    B, K, n = shape
    assert np.isfinite(Q).all() and np.isfinite(R).all() and (np.tril(R, -1) == 0).all()
    # log R_kk is the device's log of the R_kk it wrote: the host's log of that double, to the last bits of two libraries
    assert np.allclose(logr, np.log(np.einsum("bkk->bk", R)), rtol=1e-14, atol=1e-15)
    Q32, R32, lr32 = (t.double().numpy() for t in tg.mgs(torch.from_numpy(v), torch.float32))
    # Q R is the input
    own2, ownm = tr.rel_l2(_reconstruct(Q32, R32), v), tr.rel_max(_reconstruct(Q32, R32), v)
    e2, em = tr.rel_l2(_reconstruct(Q, R), v), tr.rel_max(_reconstruct(Q, R), v)
    print(shape, family, "Q R: rel-L2 %.2e (own %.2e) rel-max %.2e (own %.2e)" % (e2, own2, em, ownm))
    assert e2 <= max(ORTH_TOL, 3 * own2) and em <= max(ORTH_TOL, 3 * ownm), (e2, own2, em, ownm)
    # Q^T Q = I as well as the fp32 statement reaches it on the same input
    d, d32 = _gram_defect(Q), _gram_defect(Q32)
    print(shape, family, "|Q^T Q - I| %.2e (fp32 statement %.2e)" % (d, d32))
    assert d <= 3 * d32, (d, d32)
    if offset:
        Qa, Ra, la = _orth(v)
        assert np.array_equal(Q, Qa) and np.array_equal(R, Ra) and np.array_equal(logr, la)      # the alignment changes no bit
    if family == "normal" and 2 * K <= n:
        Q64, R64, lr64 = (t.numpy() for t in tg.mgs(torch.from_numpy(v)))
        for name, ours, ref, own in (("Q", Q, Q64, Q32), ("log R_kk", logr, lr64, lr32)):
            o2, om = tr.rel_l2(own, ref), tr.rel_max(own, ref)
            e2, em = tr.rel_l2(ours, ref), tr.rel_max(ours, ref)
            print(shape, name, "vs float64: rel-L2 %.2e (own %.2e) rel-max %.2e (own %.2e)" % (e2, o2, em, om))
            assert e2 <= max(ORTH_TOL, 3 * o2) and em <= max(ORTH_TOL, 3 * om), (name, e2, o2, em, om)


def test_orthonormalize_zero_vector_and_accumulation():
    _need_gpu()
    from lns_amd import engine
    v = tg.orth_input((2, 3, 32))
    v[:, 1] = 0
    Q, R, logr = _orth(v)
    assert not np.isnan(Q).any() and not np.isnan(R).any() and not np.isnan(logr).any()
    assert (Q[:, 1] == 0).all() and np.isneginf(logr[:, 1]).all() and np.isfinite(logr[:, [0, 2]]).all()
    assert _gram_defect(Q[:, [0, 2]]) < 1e-6
    # logr_acc accumulates over calls; without outputs the vectors get the same bits
    a, b = tg.orth_input((2, 3, 32), seed=1), tg.orth_input((2, 3, 32), seed=2)
    _, _, la = _orth(a)
    Qb, _, lb = _orth(b)
    acc = torch.zeros((2, 3), dtype=torch.float64, device="cuda")
    engine.orthonormalize(torch.from_numpy(a).cuda(), logr_acc=acc)
    qb, r_none = engine.orthonormalize(torch.from_numpy(b).cuda(), logr_acc=acc)
    bare, _ = engine.orthonormalize(torch.from_numpy(b).cuda())
    torch.cuda.synchronize()
    assert r_none is None and np.array_equal(acc.cpu().numpy(), la + lb)
    assert np.array_equal(qb.double().cpu().numpy(), Qb) and torch.equal(bare, qb)


# ---- Lyapunov exponents -----------------------------------------------------------------------------------------------------
SEED = 1234


def _gen():
    return torch.Generator(device="cuda").manual_seed(SEED)


def _lyap_setup(case):
    from lns_amd import tangent
    name, B, T, h, w = case
    model = tr.grid_model(name)
    model._owner._eng.set_option("train_wgrad", 0)
    z0, prm, _ = tg.case_start(case, 1)
    return tangent.TangentRollout(model), torch.from_numpy(z0).cuda(), torch.from_numpy(prm).cuda() if prm is not None else None, z0, prm


@pytest.mark.parametrize("spec", tg.LYAPUNOV, ids=lambda s: "%s-K%d-renorm%d" % (tr.case_id(s[0]), s[1], s[2]))
def test_lyapunov_against_the_float64_loop(spec):
    """|exponent - float64 loop's| <= max(1e-4, 3 x |float32 loop's - float64 loop's|), from the same start vectors."""
    _need_gpu()
    case, K, renorm = spec
    name, B, T, h, w = case
    roll, z0, p, z0_np, prm_np = _lyap_setup(case)
    res = roll.lyapunov(z0, T, k=K, renorm=renorm, param=p, generator=_gen())
    V0 = torch.randn((B, K) + tuple(z0.shape[1:]), dtype=torch.float32, device="cuda", generator=_gen()).cpu()
    torch.cuda.synchronize()
    ref = {}
    for dtype in (torch.float64, torch.float32):
        t = lambda a: torch.from_numpy(a).to(dtype) if a is not None else None      # noqa: E731
        ref[dtype] = tg.lyapunov(lf.propagator(name, dtype), t(z0_np), t(prm_np), V0.to(dtype), T, renorm)
    e64 = ref[torch.float64][0].numpy()
    own = float(np.abs(ref[torch.float32][0].double().numpy() - e64).max())
    ours, hist = res.exponents.cpu().numpy(), res.history.cpu().numpy()
    assert ours.shape == (B, K) and hist.shape == (T // renorm, B, K) and ours.dtype == np.float64
    err = float(np.abs(ours - e64).max())
    print(spec, "exponents %.4g .. %.4g, |diff| %.2e, own %.2e" % (e64.min(), e64.max(), err, own))
    assert np.isfinite(ours).all() and err <= max(1e-4, 3 * own), (err, own)
    assert np.allclose(ours, hist.sum(0) / T, rtol=0, atol=1e-12)          # the history's rows are the terms of the mean
    assert res.vectors.shape == (B, K) + tuple(z0.shape[1:]) and _gram_defect(res.vectors.reshape(B, K, -1).cpu().numpy()) < 1e-5
    assert tr.rel_l2(res.z_last.cpu().numpy(), ref[torch.float64][3].numpy()) <= 1e-4


def test_lyapunov_chunking_and_burn_in_are_bitwise():
    _need_gpu()
    case, K = ("E3", 2, 6, 4, 4), 4
    roll, z0, p, _, _ = _lyap_setup(case)
    T = case[2]
    for renorm in (1, 2):
        full = roll.lyapunov(z0, T, k=K, renorm=renorm, generator=_gen())
        for chunk in (2, 4, 5):          # 5: a chunk boundary inside a renormalisation interval (renorm 2), and a short last chunk
            part = roll.lyapunov(z0, T, k=K, renorm=renorm, chunk=chunk, generator=_gen())
            for a, b in zip(full, part):
                assert torch.equal(a, b), (renorm, chunk)
        late = roll.lyapunov(z0, T, k=K, renorm=renorm, burn_in=2, generator=_gen())
        assert torch.equal(late.history, full.history[2 // renorm:])                 # exactly the leading rows are dropped
        assert torch.equal(late.vectors, full.vectors) and torch.equal(late.z_last, full.z_last)
        assert torch.allclose(late.exponents, late.history.sum(0) / (T - 2), rtol=0, atol=1e-12)
    half = roll.lyapunov(z0, T, k=K, generator=_gen(), dt=0.5)
    assert torch.equal(half.exponents, roll.lyapunov(z0, T, k=K, generator=_gen()).exponents / 0.5)


def test_latent_dynamics_lyapunov_end_to_end():
    """The drop-in on the ns2d_mini preset: encode, run; finite and reproducible under a seeded generator."""
    _need_gpu()
    from lns_amd import filler
    model = tr.grid_model("E3")
    model._owner._eng.set_option("train_wgrad", 0)
    a = model.args
    x = torch.from_numpy(filler.normal("x", (2, a.in_channels, a.Ly, a.Lx), 7)).cuda()
    r1 = model.lyapunov(x, 4, k=3, renorm=2, generator=_gen())
    r2 = model.lyapunov(x, 4, k=3, renorm=2, generator=_gen())
    torch.cuda.synchronize()
    assert r1.exponents.shape == (2, 3) and torch.isfinite(r1.exponents).all() and torch.isfinite(r1.vectors).all()
    for t1, t2 in zip(r1, r2):
        assert torch.equal(t1, t2)
    c, h, w = model._owner._eng.latent_shape()
    assert r1.vectors.shape == (2, 3, c, h, w) and r1.z_last.shape == (2, c, h, w) and r1.history.shape == (2, 2, 3)

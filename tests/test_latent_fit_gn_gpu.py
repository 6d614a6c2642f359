"""GPU: the Gauss-Newton latent fit -- lns_train_gn_product, lns_op_cg_start / lns_op_cg_update, lns_fit_gn_step,
LatentFit.run_gauss_newton / hessian_product and LatentDynamics.assimilate(method="gauss_newton").

  * H v and v^T H v against torch.func.jvp + vjp in float64 (tests/latent_fit_gn_reference.py) within latent_fit_reference.rule --
    max(1e-4, 3 x the float32 statement's own error) in rel-L2 and rel-max -- on latent_fit_reference.ADJOINT_CASES, with and
    without background / damping, under both "train_wgrad" values;
  * symmetry, ours against ours: |<u, H v> - <v, H u>| <= 4e-4 |sqrt(W) J u| |sqrt(W) J v| -- each of the two inner products
    is the true u^T H v up to the 2e-4 of test_tangent_pairs_with_the_adjoint (tangent and adjoint each held to 1e-4) -- and
    v^T H v >= 0;
  * bits: the product is train_tangent -> the weighting -> the state-only train_backward called separately; a repeated product;
    train_tangent before and after a product (the adjoint leaves the tape and the forward packs alone); v is not modified;
  * lns_op_cg_start / lns_op_cg_update equal the order-exact float64 statement bit for bit;
  * lns_fit_gn_step is the composition of its calls bit for bit, its loss has lns_fit_step's bits, a short workspace refuses;
  * the twin experiments reach half of the float64-measured factors, with a loss that never increases;
  * assimilate(method="gauss_newton") end to end."""
import ctypes

import numpy as np
import pytest
import torch

import latent_fit_gn_reference as gn
import latent_fit_reference as lf
import train_reference as tr

pytestmark = pytest.mark.gpu
DAMPED = [(0.0, 0.0), (gn.GN_LAMBDA, gn.GN_DAMPING)]


def _need_gpu():
    assert torch.cuda.is_available(), "GPU test selected but no GPU is visible"


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda() if a is not None else None


def test_fit_gauss_newton_is_built():
    """Fails on the parent: the symbols and the feature name."""
    from lns_amd import _lib
    L = _lib.lib()
    for s in ("lns_train_gn_product_workspace_bytes", "lns_train_gn_product", "lns_op_cg_start", "lns_op_cg_update",
              "lns_fit_gn_step_workspace_bytes", "lns_fit_gn_step"):
        assert hasattr(L, s), s
    assert L.lns_build_has(b"fit_gauss_newton") == 1


def _setup(case, form=0):
    """After the training forward on the product's workspace."""
    name, B, T, h, w = case
    model = tr.grid_model(name)
    eng = model._owner._eng
    eng.set_option("train_wgrad", form)
    z0, prm, v, u = gn.case_start(case)
    steps, wts = gn.case_obs(case)
    params = {k: p.detach() for k, p in model.named_parameters() if k.startswith("propagator.")}
    z0, p, v, u = _cuda(z0), _cuda(prm), _cuda(v), _cuda(u)
    ws = torch.empty(eng.train_gn_product_workspace_bytes(B, h, w, T, len(steps)), dtype=torch.uint8, device="cuda")
    z_pred, _ = eng.train_forward(params, z0, T, param=p, workspace=ws)
    return dict(eng=eng, params=params, z0=z0, p=p, v=v, u=u, steps=steps, w=wts, ws=ws, z_pred=z_pred, T=T)


def _product(s, v, lam, mu):
    return s["eng"].train_gn_product(s["params"], s["z0"], s["z_pred"], v, s["steps"], s["ws"], weights=s["w"], background=lam, damping=mu)


# ---- parity -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", tr.FORMS)
@pytest.mark.parametrize("lam,mu", DAMPED)
@pytest.mark.parametrize("case", lf.ADJOINT_CASES, ids=tr.case_id)
def test_hv_against_float64(case, lam, mu, form):
    _need_gpu()
    s = _setup(case, form)
    keep = s["v"].clone()
    hv, vhv = _product(s, s["v"], lam, mu)
    torch.cuda.synchronize()
    assert torch.equal(s["v"], keep)                                                # v is not modified
    z_plain, _ = s["eng"].train_forward(s["params"], s["z0"], s["T"], param=s["p"])
    assert torch.equal(z_plain, s["z_pred"])                                        # the forward on the larger workspace keeps its bits
    r64, r32 = gn.product_truth(case, lam, mu)
    ours = hv.cpu().numpy()
    assert np.isfinite(ours).all() and hv.shape == s["v"].shape and vhv.dtype == torch.float64
    e2, b2, em, bm, o2, om = lf.rule(ours, r64["hv"], r32["hv"])
    print("%s form %d lam %g mu %g: hv rel-L2 %.2e/%.2e rel-max %.2e/%.2e (own %.2e %.2e)" % (tr.case_id(case), form, lam, mu, e2, b2, em, bm, o2, om))
    assert e2 <= b2, ("rel-L2", e2, b2, o2)
    assert em <= bm, ("rel-max", em, bm, om)
    e2, b2, em, bm, o2, om = lf.rule(vhv.cpu().numpy(), r64["vhv"], r32["vhv"])
    print("%s form %d lam %g mu %g: vhv rel-L2 %.2e/%.2e rel-max %.2e/%.2e (own %.2e %.2e)" % (tr.case_id(case), form, lam, mu, e2, b2, em, bm, o2, om))
    assert e2 <= b2 and em <= bm, ("vhv", e2, b2, em, bm)
    assert (vhv >= 0).all()


@pytest.mark.parametrize("lam,mu", DAMPED)
@pytest.mark.parametrize("case", lf.ADJOINT_CASES, ids=tr.case_id)
def test_operator_is_symmetric_and_not_negative(case, lam, mu):
    _need_gpu()
    s = _setup(case)
    B = case[1]
    hv, vhv = _product(s, s["v"], lam, mu)
    hu, uhu = _product(s, s["u"], lam, mu)
    torch.cuda.synchronize()
    assert (vhv >= 0).all() and (uhu >= 0).all()
    u64, v64, hv64, hu64 = (t.double().cpu().reshape(B, -1) for t in (s["u"], s["v"], hv, hu))
    r64, _ = gn.product_truth(case, lam, mu)
    n = u64.shape[1]
    cw = np.array([2.0 * wk / n for wk in s["w"]])
    scale = np.sqrt((cw[None] * (r64["ju"] ** 2).reshape(B, len(cw), -1).sum(2)).sum(1)) * \
        np.sqrt((cw[None] * (r64["jv"] ** 2).reshape(B, len(cw), -1).sum(2)).sum(1))
    # the diagonal term is symmetric by construction; its elementwise fp32 rounding: 2^-23 |u| |c_d v| at the most
    diag = (2.0 * lam / n + mu) * (u64.norm(dim=1) * v64.norm(dim=1)).numpy() * 2.0 ** -23
    defect = ((u64 * hv64).sum(1) - (v64 * hu64).sum(1)).abs().numpy()
    print(tr.case_id(case), "lam %g mu %g: symmetry defect / scale" % (lam, mu), defect / scale)
    assert (defect <= 4e-4 * scale + diag).all(), (defect, scale)


# ---- bits -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam,mu", DAMPED)
@pytest.mark.parametrize("case", [("E3", 4, 5, 8, 8), ("E6", 5, 2, 7, 15), ("E5", 3, 1, 1, 130)], ids=tr.case_id)
def test_product_is_its_parts_bit_for_bit(case, lam, mu):
    _need_gpu()
    s = _setup(case)
    eng, params, T = s["eng"], s["params"], s["T"]
    B = case[1]
    v = s["v"]
    keep = v.clone()

    def tangent():
        vv = v.clone()[:, None].contiguous()
        return eng.train_tangent(params, vv, T, s["ws"], keep=True)
    jv_before = tangent()
    hv, vhv = _product(s, v, lam, mu)
    jv_after = tangent()
    hv2, vhv2 = _product(s, v, lam, mu)
    assert torch.equal(jv_before, jv_after)                      # the adjoint and its weight repack leave the tape and the forward packs alone
    assert torch.equal(hv, hv2) and torch.equal(vhv, vhv2)       # a repeated product on one tape
    assert torch.equal(v, keep)
    # the parts: the tangent, the weighting (one fp32 multiplication, zeros elsewhere), the state-only adjoint, the diagonal term
    n = v[0].numel()
    cot = torch.zeros_like(s["z_pred"])
    for k, t in enumerate(s["steps"]):
        cot[:, t] = jv_before[:, 0, t] * float(np.float32(2.0 * s["w"][k] / n))
    _, gz = eng.train_backward(params, s["z0"], s["z_pred"], cot, s["ws"], need_z_grad=True, state_only=True)
    c_d = float(np.float32(2.0 * lam / n + mu))
    if c_d != 0.0:
        cv = v * c_d
        gz = gz + cv
    torch.cuda.synchronize()
    assert torch.equal(hv, gz)
    # vhv: the tangent side, summed in float64 on the host (another order: to rounding of a double sum)
    j64 = jv_before[:, 0].double().cpu().reshape(B, T, -1)
    ref = sum((2.0 * s["w"][k] / n) * (j64[:, t] ** 2).sum(1) for k, t in enumerate(s["steps"])) \
        + (2.0 * lam / n + mu) * (v.double().cpu().reshape(B, -1) ** 2).sum(1)
    assert torch.allclose(vhv.cpu(), ref, rtol=1e-12, atol=0)


# ---- conjugate gradients ------------------------------------------------------------------------------------------------------
def _buffers(B, n, offset, k):
    """k fp32 [B, n] device tensors; offset: each starts one float past an aligned allocation."""
    out = []
    for _ in range(k):
        buf = torch.zeros(B * n + 1, dtype=torch.float32, device="cuda")
        t = buf[1:].view(B, n) if offset else buf[:B * n].view(B, n)
        assert t.is_contiguous() and (not offset or t.data_ptr() % 8 == 4)
        out.append(t)
    return out


@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "offset"])
@pytest.mark.parametrize("given", [False, True], ids=["php-computed", "php-given"])
@pytest.mark.parametrize("shape", gn.CG_SHAPES, ids=lambda s: "B%d-n%d" % s)
def test_cg_equals_the_order_exact_statement(shape, given, offset):
    """Four steps on a diagonal operator hp = d * p (formed on the host from the device's p, so both sides see the same hp); with
    B = 3 sample 1 has g = 0 and stays frozen among active ones; then a step the tolerance freezes."""
    _need_gpu()
    from lns_amd import engine, filler
    B, n = shape
    g_np = filler.normal("cg_g", (B, n), 11)
    d_np = (0.25 + np.abs(filler.normal("cg_d", (B, n), 12))).astype(np.float32)
    if B > 1:
        g_np[1] = 0
    g, x, r, p, hp = _buffers(B, n, offset, 5)
    g.copy_(torch.from_numpy(g_np))
    x.fill_(7.0)                                                   # cg_start writes every element
    rs, rs0 = engine.cg_start(g, x, r, p)
    applied = torch.zeros(B, dtype=torch.int32, device="cuda")
    sx, sr, sp, srs, srs0 = gn.cg_start(g_np)
    sapp = None

    def same():
        torch.cuda.synchronize()
        for ours, ref, what in ((x, sx, "x"), (r, sr, "r"), (p, sp, "p")):
            assert np.array_equal(ours.cpu().numpy().view(np.uint32), ref.view(np.uint32)), what
        assert np.array_equal(rs.cpu().numpy().view(np.uint64), srs.view(np.uint64)), (rs.cpu().numpy(), srs)
        assert np.array_equal(rs0.cpu().numpy().view(np.uint64), srs0.view(np.uint64))
    same()
    for it in range(4):
        hp_np = d_np * sp                                          # one fp32 multiplication
        hp.copy_(torch.from_numpy(hp_np))
        php_np = None
        if given:                                                  # the caller's value: here, another number than <p, hp>
            php_np = np.array([1.25 * gn.block_sum(sp[b].astype(np.float64) * hp_np[b].astype(np.float64)) for b in range(B)])
        engine.cg_update(x, r, p, hp, rs, rs0, php=_cuda(php_np), applied=applied)
        sx, sr, sp, srs, sapp = gn.cg_update(sx, sr, sp, hp_np, srs, srs0, php=php_np, applied=sapp)
        same()
        assert np.array_equal(applied.cpu().numpy(), sapp)
    expect = sapp.tolist()                                        # (n = 1 converges in one step: rs = 0 freezes the rest)
    assert expect[0] >= 1 and (n == 1 or expect[0] == 4), expect
    if B > 1:
        assert expect[1] == 0 and (sx[1] == 0).all() and not np.isnan(x.cpu().numpy()).any()
    # the tolerance: |r| <= 1 * |r0| holds for every sample, nothing is written
    hp.copy_(torch.from_numpy(d_np * sp))
    engine.cg_update(x, r, p, hp, rs, rs0, tol=1.0, applied=applied)
    same()
    assert applied.cpu().numpy().tolist() == expect
    # php = 0 and php = NaN freeze as well
    for bad in (0.0, float("nan")):
        engine.cg_update(x, r, p, hp, rs, rs0, php=torch.full((B,), bad, dtype=torch.float64, device="cuda"), applied=applied)
        same()
    assert applied.cpu().numpy().tolist() == expect


# ---- the whole step ---------------------------------------------------------------------------------------------------------
def _twin(setup):
    d = lf.twin(setup)
    model = tr.grid_model(setup[0])
    model._owner._eng.set_option("train_wgrad", 0)
    return d, model


@pytest.mark.parametrize("lam,mu", DAMPED)
@pytest.mark.parametrize("setup", [("E6", 3, 3, 2, 2), ("E3", 3, 3, 4, 4)], ids=tr.case_id)
def test_gn_step_is_the_composition_of_its_calls(setup, lam, mu):
    _need_gpu()
    from lns_amd import _lib, engine
    d, model = _twin(setup)
    eng = model._owner._eng
    params = {k: p.detach() for k, p in model.named_parameters() if k.startswith("propagator.")}
    obs, p, zb = _cuda(d["obs"]), _cuda(d["p_true"]), (_cuda(d["z_true"]) if lam > 0 else None)
    steps, w = lf.TWIN_STEPS, lf.TWIN_WEIGHTS
    B, T, n_cg, outer = setup[1], steps[-1] + 1, 3, 2
    h, wd = setup[3], setup[4]
    spec = engine.gn_spec(steps, w, lam, n_cg=n_cg, damping=mu)
    # (a) the fused call
    z = _cuda(d["z_start"])
    fused = [tuple(t.clone() for t in eng.fit_gn_step(params, z, obs, spec, param=p, z_background=zb)) for _ in range(outer)]
    # (b) the separate calls
    z2 = _cuda(d["z_start"])
    ws = torch.empty(eng.train_gn_product_workspace_bytes(B, h, wd, T, len(steps)), dtype=torch.uint8, device="cuda")
    for it in range(outer):
        z_pred, _ = eng.train_forward(params, z2, T, param=p, workspace=ws)
        bg = dict(z0=z2, z_background=zb, background=lam) if zb is not None else {}
        loss, per, g, gbg = engine.obs_loss(z_pred, obs, steps, w, **bg)
        _, gz = eng.train_backward(params, z2, z_pred, g, ws, need_z_grad=True, state_only=True)
        if gbg is not None:
            gz = gz + gbg
        x, r, pp = torch.empty_like(gz), torch.empty_like(gz), torch.empty_like(gz)
        rs, rs0 = engine.cg_start(gz, x, r, pp)
        applied = torch.zeros(B, dtype=torch.int32, device="cuda")
        for _ in range(n_cg):
            hp, vhv = eng.train_gn_product(params, z2, z_pred, pp, steps, ws, weights=w, background=lam, damping=mu)
            engine.cg_update(x, r, pp, hp, rs, rs0, php=vhv, applied=applied)
        z2 = z2 + x
        torch.cuda.synchronize()
        f_loss, f_per, f_resid, f_applied = fused[it]
        assert torch.equal(loss, f_loss) and torch.equal(per, f_per), it
        assert torch.equal(applied, f_applied) and (applied == n_cg).all(), (it, applied)
        resid = torch.sqrt(rs / rs0)
        assert torch.allclose(f_resid.double(), resid, rtol=1e-6, atol=0), (f_resid, resid)
        assert (f_resid < 1).all()
    assert torch.equal(z, z2) and not torch.equal(z, _cuda(d["z_start"]))
    # loss and per of the first iteration: lns_fit_step's bits for the same z0
    za = _cuda(d["z_start"])
    gz_, mz_, vz_ = [torch.zeros_like(za) for _ in range(3)]
    a_loss, a_per = eng.fit_step(params, za, obs, engine.fit_spec(steps, w, lam, state=engine.update_spec(lf.LR_STATE)), param=p,
                                 z_background=zb, g_z=gz_, exp_avg_z=mz_, exp_avg_sq_z=vz_)
    torch.cuda.synchronize()
    assert torch.equal(a_loss, fused[0][0]) and torch.equal(a_per, fused[0][1])
    # a short workspace refuses with the byte count and touches nothing
    need = eng.fit_gn_step_workspace_bytes(B, h, wd, T, len(steps))
    big = torch.empty(need, dtype=torch.uint8, device="cuda")
    zk = z.clone()
    lossk = torch.full((B,), -3.0, device="cuda")
    rc = eng._L.lns_fit_gn_step(eng._h, eng._ptr_array(params), zk.data_ptr(), eng._ptr(p), obs.data_ptr(), eng._ptr(zb), B, h, wd,
                                ctypes.byref(spec), lossk.data_ptr(), None, None, None, big.data_ptr(), need - 1, eng._stream(zk))
    assert rc == _lib.LNS_ENOMEM and str(need) in eng._L.lns_last_error(eng._h).decode()
    torch.cuda.synchronize()
    assert torch.equal(zk, z) and (lossk == -3.0).all()


@pytest.mark.parametrize("outer", [1, 3])
@pytest.mark.parametrize("setup", lf.TWINS, ids=tr.case_id)
def test_twin_experiment(setup, outer):
    """Worst-sample loss[0] / loss[-1] is at least half of the float64-measured factor (latent_fit_gn_reference.MEASURED); the
    loss never increases."""
    _need_gpu()
    from lns_amd import fit
    d, model = _twin(setup)
    B = setup[1]
    z_start, p = _cuda(d["z_start"]), _cuda(d["p_true"])
    keep_z, keep_p = z_start.clone(), (p.clone() if p is not None else None)
    fitter = fit.LatentFit(model)
    res = fitter.run_gauss_newton(z_start, _cuda(d["obs"]), lf.TWIN_STEPS, param=p, weights=lf.TWIN_WEIGHTS, outer=outer,
                                  cg_iters=gn.CG_ITERS)
    assert res.loss.shape == (outer + 1, B) and res.per.shape == (B, len(lf.TWIN_STEPS)) and res.loss.is_cuda
    assert torch.equal(z_start, keep_z) and (p is None or (torch.equal(p, keep_p) and torch.equal(res.param, p)))
    assert res.z0.data_ptr() != z_start.data_ptr()
    loss = res.loss.cpu().numpy()
    red = loss[0] / loss[-1]
    want = gn.GPU_FRACTION * gn.MEASURED[(outer, gn.CG_ITERS)][setup]
    print(tr.case_id(setup), "%d x %d: loss" % (outer, gn.CG_ITERS), loss, "reduction", red, "asked", want)
    assert (np.diff(loss, axis=0) <= 0).all(), loss
    assert (red >= want).all(), (red, want)
    e0 = np.sqrt(((d["z_start"] - d["z_true"]).astype(np.float64) ** 2).reshape(B, -1).sum(1))
    e1 = np.sqrt(((res.z0.cpu().numpy() - d["z_true"]).astype(np.float64) ** 2).reshape(B, -1).sum(1))
    print(tr.case_id(setup), "state error / start's", e1 / e0)


def test_hessian_product_runs_one_product_per_vector():
    _need_gpu()
    from lns_amd import fit
    case = ("E6", 5, 2, 7, 15)
    s = _setup(case)
    model = tr.grid_model(case[0])
    vs = torch.stack([s["v"], s["u"]], 1)
    hv, vhv = fit.LatentFit(model, background=gn.GN_LAMBDA).hessian_product(s["z0"], vs, s["steps"], param=s["p"], weights=s["w"],
                                                                           damping=gn.GN_DAMPING)
    assert hv.shape == vs.shape and vhv.shape == (case[1], 2) and vhv.dtype == torch.float64
    a, av = _product(s, s["v"], gn.GN_LAMBDA, gn.GN_DAMPING)
    b, bv = _product(s, s["u"], gn.GN_LAMBDA, gn.GN_DAMPING)
    torch.cuda.synchronize()
    assert torch.equal(hv[:, 0], a) and torch.equal(hv[:, 1], b) and torch.equal(vhv[:, 0], av) and torch.equal(vhv[:, 1], bv)


@pytest.mark.parametrize("name", ["E3", "E6"])
def test_assimilate_gauss_newton_end_to_end(name):
    """ns2d_mini and the conditional preset: shapes, the caller's tensors unchanged, finite results (random frames are not data
    the model can reach, and there is no line search: no decrease is promised here -- the twin experiments ask for it), and the
    refusal of a parameter fit."""
    _need_gpu()
    from lns_amd import filler
    from lns_amd._lib import LnsError
    model = tr.grid_model(name)
    model._owner._eng.set_option("train_wgrad", 0)
    args = model.args
    cond = tr.ENGINES[name]["family"] == "twophase_cond"
    B, steps = 2, [0, 2]
    x0 = _cuda(filler.normal("assim_x0", (B, args.in_channels, args.Ly, args.Lx), tr.INPUT_SEED))
    y = _cuda(filler.normal("assim_y", (B, len(steps), args.in_channels, args.Ly, args.Lx), tr.INPUT_SEED))
    prm = (_cuda(filler.uniform01("assim_p", B, tr.INPUT_SEED).astype(np.float32)),) if cond else ()
    keep = [t.clone() for t in (x0, y) + prm]
    res = model.assimilate(x0, y, steps, *prm, method="gauss_newton", outer=2, cg_iters=4, damping=1e-3)
    torch.cuda.synchronize()
    for t, k in zip((x0, y) + prm, keep):
        assert torch.equal(t, k)
    c, h, w = model._owner._eng.latent_shape()
    assert res.z0.shape == (B, c, h, w) and res.loss.shape == (3, B) and res.per.shape == (B, len(steps))
    assert (res.param is None) == (not cond) and (not cond or torch.equal(res.param, prm[0]))
    loss = res.loss.cpu().numpy()
    print(name, "assimilate gauss_newton loss", loss)
    assert np.isfinite(loss).all() and np.isfinite(res.z0.cpu().numpy()).all(), loss
    if cond:
        with pytest.raises(LnsError, match="no param direction"):
            model.assimilate(x0, y, steps, *prm, method="gauss_newton", fit_param=True)

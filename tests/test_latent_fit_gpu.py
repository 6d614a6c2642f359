"""GPU: the latent fit -- lns_fit_step, lns_amd.fit.LatentFit and LatentDynamics.assimilate.

  * K = 5 calls of lns_fit_step equal, bit for bit, K compositions of the separate calls (train_forward, obs_loss, the
    state-only train_backward, the add, lns_update_step_tensors), fitting the state, `param` or both, with and without the
    background term;
  * one step from the reference's start: g_z and g_p against float64 under the gradient rule max(GRAD_TOL, 3 x own) in
    rel-L2 and rel-max (the update itself is update_multi_kernel's, covered by tests/test_train_clip_gpu.py);
  * the twin experiments of tests/latent_fit_reference.py, 40 iterations: every sample's loss and param error fall by at
    least latent_fit_reference.GPU_* -- at most half of what the float64 statement measures (tests/test_latent_fit_cpu.py).
    No step-by-step comparison of trajectories: Adam's first steps are sign-like where a gradient is at rounding level,
    which makes an elementwise gate flaky by construction;
  * a sample fitted in a batch of three agrees with the same sample fitted alone;
  * LatentFit.run leaves the caller's z0 / param as they were; assimilate lowers the observation loss of the plain encoding."""
import ctypes

import numpy as np
import pytest
import torch

import latent_fit_reference as lf
import train_reference as tr

pytestmark = pytest.mark.gpu


def _need_gpu():
    assert torch.cuda.is_available(), "GPU test selected but no GPU is visible"


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda() if a is not None else None


def _twin(setup):
    d = lf.twin(setup)
    model = tr.grid_model(setup[0])
    model._owner._eng.set_option("train_wgrad", 0)
    return d, model


def _update(L, t, g, m, v, spec, stream):
    one = lambda x: (ctypes.c_void_p * 1)(x.data_ptr())        # noqa: E731
    rc = L.lns_update_step_tensors(1, one(t), one(g), one(m), one(v), (ctypes.c_int64 * 1)(t.numel()), ctypes.byref(spec), None, stream)
    assert rc == 0, L.lns_create_error()


@pytest.mark.parametrize("lam", [0.0, 0.3])
@pytest.mark.parametrize("mode", ["state", "param", "both"])
def test_fit_step_is_the_composition_of_its_calls(mode, lam):
    _need_gpu()
    from lns_amd import engine
    setup = ("E6", 3, 3, 2, 2)
    d, model = _twin(setup)
    eng = model._owner._eng
    fit_z, fit_p = mode != "param", mode != "state"
    params = {k: p.detach() for k, p in model.named_parameters() if k.startswith("propagator.")}
    obs, zb = _cuda(d["obs"]), (_cuda(d["z_true"]) if lam > 0 else None)
    steps, w = lf.TWIN_STEPS, lf.TWIN_WEIGHTS
    stream = eng._stream(obs)

    def state():
        z, p = _cuda(d["z_start"]), _cuda(d["p_start"])
        return z, p, [torch.zeros_like(z) for _ in range(3)], [torch.zeros_like(p) for _ in range(3)]
    # (a) the fused call
    z, p, (gz, mz, vz), (gp, mp, vp) = state()
    losses, pers = [], []
    for it in range(5):
        spec = engine.fit_spec(steps, w, lam, state=engine.update_spec(lf.LR_STATE, step=it + 1) if fit_z else None,
                               param=engine.update_spec(lf.LR_PARAM, step=it + 1) if fit_p else None)
        kw = dict(g_z=gz, exp_avg_z=mz, exp_avg_sq_z=vz) if fit_z else {}
        if fit_p:
            kw.update(g_p=gp, exp_avg_p=mp, exp_avg_sq_p=vp)
        loss, per = eng.fit_step(params, z, obs, spec, param=p, z_background=zb, **kw)
        losses.append(loss); pers.append(per)
    # (b) the separate calls
    z2, p2, (gz2, mz2, vz2), (gp2, mp2, vp2) = state()
    for it in range(5):
        z_pred, ws = eng.train_forward(params, z2, steps[-1] + 1, param=p2)
        bg = dict(z0=z2, z_background=zb, background=lam, need_bg_grad=fit_z) if zb is not None else {}
        loss, per, g, gbg = engine.obs_loss(z_pred, obs, steps, w, **bg)
        out = eng.train_backward(params, z2, z_pred, g, ws, need_z_grad=fit_z, need_param_grad=fit_p, state_only=True)
        assert out[0] == {}
        if fit_z:
            gz2 = out[1] + gbg if gbg is not None else out[1]
            _update(eng._L, z2, gz2, mz2, vz2, engine.update_spec(lf.LR_STATE, step=it + 1), stream)
        if fit_p:
            gp2 = out[2]
            _update(eng._L, p2, gp2, mp2, vp2, engine.update_spec(lf.LR_PARAM, step=it + 1), stream)
        assert torch.equal(loss, losses[it]) and torch.equal(per, pers[it]), it
    torch.cuda.synchronize()
    assert torch.equal(z, z2) and torch.equal(p, p2)
    if fit_z:
        assert torch.equal(gz, gz2) and torch.equal(mz, mz2) and torch.equal(vz, vz2)
        assert not torch.equal(z, _cuda(d["z_start"]))
    else:
        assert torch.equal(z, _cuda(d["z_start"]))
    if fit_p:
        assert torch.equal(gp, gp2) and torch.equal(mp, mp2) and torch.equal(vp, vp2)
        assert not torch.equal(p, _cuda(d["p_start"]))
    else:
        assert torch.equal(p, _cuda(d["p_start"]))


@pytest.mark.parametrize("setup", lf.TWINS, ids=tr.case_id)
def test_fit_step_gradients_match_float64(setup):
    _need_gpu()
    from lns_amd import engine
    d, model = _twin(setup)
    eng = model._owner._eng
    cond = d["p_start"] is not None
    params = {k: p.detach() for k, p in model.named_parameters() if k.startswith("propagator.")}
    z, p, obs, zb = _cuda(d["z_start"]), _cuda(d["p_start"]), _cuda(d["obs"]), _cuda(d["z_true"])
    lam = 0.3
    gz, mz, vz = [torch.zeros_like(z) for _ in range(3)]
    kw = dict(g_z=gz, exp_avg_z=mz, exp_avg_sq_z=vz)
    if cond:
        gp, mp, vp = [torch.zeros_like(p) for _ in range(3)]
        kw.update(g_p=gp, exp_avg_p=mp, exp_avg_sq_p=vp)
    spec = engine.fit_spec(lf.TWIN_STEPS, lf.TWIN_WEIGHTS, lam, state=engine.update_spec(lf.LR_STATE),
                           param=engine.update_spec(lf.LR_PARAM) if cond else None)
    loss, per = eng.fit_step(params, z, obs, spec, param=p, z_background=zb, **kw)
    refs = []
    for dt in (torch.float64, torch.float32):
        to = lambda a: torch.from_numpy(a).to(dt) if a is not None else None      # noqa: E731
        refs.append(lf.fit_grads(lf.propagator(setup[0], dt), to(d["z_start"]), to(d["p_start"]), to(d["obs"]), lf.TWIN_STEPS,
                                 lf.TWIN_WEIGHTS, to(d["z_true"]), lam))
    r64, r32 = refs
    for ours, k in ((gz, "g_z"), (gp, "g_p")) if cond else ((gz, "g_z"),):
        e2, b2, em, bm, o2, om = lf.rule(ours.cpu().numpy(), r64[k].numpy(), r32[k].double().numpy())
        print("%s %s: rel-L2 %.2e/%.2e rel-max %.2e/%.2e (own %.2e %.2e)" % (tr.case_id(setup), k, e2, b2, em, bm, o2, om))
        assert e2 <= b2 and em <= bm, (k, e2, b2, em, bm)
    for ours, k in ((loss, "loss"), (per, "per")):
        e2 = tr.rel_max(ours.cpu().numpy(), r64[k].numpy())
        assert e2 <= max(tr.GRAD_TOL, 3 * tr.rel_max(r32[k].double().numpy(), r64[k].numpy())), (k, e2)


@pytest.mark.parametrize("setup", lf.TWINS, ids=tr.case_id)
def test_twin_experiment(setup):
    _need_gpu()
    from lns_amd import fit
    d, model = _twin(setup)
    cond = d["p_start"] is not None
    z_start, p_start = _cuda(d["z_start"]), _cuda(d["p_start"])
    keep_z, keep_p = z_start.clone(), (p_start.clone() if cond else None)
    fitter = fit.LatentFit(model, lr_state=lf.LR_STATE, lr_param=lf.LR_PARAM)
    assert fitter.fit_param == cond
    res = fitter.run(z_start, _cuda(d["obs"]), lf.TWIN_STEPS, param=p_start, weights=lf.TWIN_WEIGHTS, iters=lf.TWIN_ITERS)
    assert res.loss.shape == (lf.TWIN_ITERS, setup[1]) and res.per.shape == (setup[1], len(lf.TWIN_STEPS)) and res.loss.is_cuda
    # the caller's tensors keep their values
    assert torch.equal(z_start, keep_z) and (not cond or torch.equal(p_start, keep_p))
    assert res.z0.data_ptr() != z_start.data_ptr()
    loss = res.loss.cpu().numpy()
    red = loss[0] / loss[-1]
    print(tr.case_id(setup), "loss reduction", red)
    assert (red >= lf.GPU_LOSS_RED).all(), red
    if cond:
        e1 = np.abs(res.param.cpu().numpy() - d["p_true"])
        print(tr.case_id(setup), "param error", lf.PARAM_OFFSET, "->", e1)
        assert (e1 <= lf.PARAM_OFFSET / lf.GPU_PARAM_RED[setup]).all(), e1
        # the state known, only param fitted
        only = fit.LatentFit(model, lr_param=lf.LR_PARAM, fit_state=False).run(_cuda(d["z_true"]), _cuda(d["obs"]), lf.TWIN_STEPS,
                                                                               param=p_start, weights=lf.TWIN_WEIGHTS, iters=lf.TWIN_ITERS)
        assert torch.equal(only.z0, _cuda(d["z_true"]))
        e2 = np.abs(only.param.cpu().numpy() - d["p_true"])
        print(tr.case_id(setup), "param error, state known", lf.PARAM_OFFSET, "->", e2)
        assert (e2 <= lf.PARAM_OFFSET / lf.GPU_PARAM_ONLY_RED).all(), e2


def test_a_sample_fits_alone_as_in_a_batch():
    """5 iterations; the difference between a sample's latent (param) fitted in the batch of three and fitted alone, relative
    to the distance it moved, stays within max(1e-4, 3 x the same figure of the float32 CPU statement)."""
    _need_gpu()
    from lns_amd import fit
    setup = ("E6", 3, 3, 7, 15)
    d, model = _twin(setup)
    fitter = fit.LatentFit(model, lr_state=lf.LR_STATE, lr_param=lf.LR_PARAM)
    z_start, p_start, obs = _cuda(d["z_start"]), _cuda(d["p_start"]), _cuda(d["obs"])
    both = fitter.run(z_start, obs, lf.TWIN_STEPS, param=p_start, weights=lf.TWIN_WEIGHTS, iters=5)
    prop32 = lf.propagator(setup[0], torch.float32)
    f32 = lambda a: torch.from_numpy(a)      # noqa: E731
    zb32, pb32, _ = lf.fit(prop32, f32(d["z_start"]), f32(d["p_start"]), f32(d["obs"]), lf.TWIN_STEPS, lf.TWIN_WEIGHTS, iters=5)

    def figure(a, alone, start):
        a, alone, start = (t.double().cpu().numpy() for t in (a, alone, start))
        return float(np.sqrt(((a - alone) ** 2).sum() / ((alone - start) ** 2).sum()))
    for b in range(setup[1]):
        s = slice(b, b + 1)
        one = fitter.run(z_start[s], obs[s], lf.TWIN_STEPS, param=p_start[s], weights=lf.TWIN_WEIGHTS, iters=5)
        z1, p1, _ = lf.fit(prop32, f32(d["z_start"][s]), f32(d["p_start"][s]), f32(d["obs"][s]), lf.TWIN_STEPS, lf.TWIN_WEIGHTS, iters=5)
        for ours, alone, start, ref_b, ref_1, ref_start, what in (
                (both.z0[s], one.z0, z_start[s], zb32[s], z1, f32(d["z_start"][s]), "z0"),
                (both.param[s], one.param, p_start[s], pb32[s], p1, f32(d["p_start"][s]), "param")):
            fig, own = figure(ours, alone, start), figure(ref_b, ref_1, ref_start)
            print("sample %d %s: %.3g (float32 statement %.3g)" % (b, what, fig, own))
            assert fig <= max(1e-4, 3 * own), (b, what, fig, own)


def test_assimilate_lowers_the_observation_loss_of_the_encoding():
    _need_gpu()
    import gpu_checks as gc
    from lns_amd import config, filler
    args = config.preset("ns2d_mini")
    model, _ = gc.build_models(args, tr.WEIGHT_SEED)
    B, steps = 2, [0, 2]
    x0 = _cuda(filler.normal("assim_x0", (B, args.in_channels, args.Ly, args.Lx), tr.INPUT_SEED))
    y = _cuda(filler.normal("assim_y", (B, len(steps), args.in_channels, args.Ly, args.Lx), tr.INPUT_SEED))
    res = model.assimilate(x0, y, steps, iters=10)
    z_enc = model.x_to_z(x0)
    assert res.z0.shape == z_enc.shape and not torch.equal(res.z0, z_enc)
    eng = model._engine(z_enc)
    z_obs = model.x_to_z(y.reshape((B * len(steps),) + tuple(y.shape[2:]))).reshape((B, len(steps)) + tuple(z_enc.shape[1:]))

    def obs_loss_of(z0):
        zp, _ = eng.rollout_latent(z0, steps[-1] + 1, to_x=False)
        return lf.obs_loss(zp.double().cpu(), z_obs.double().cpu(), steps)[0].numpy()
    before, after = obs_loss_of(z_enc), obs_loss_of(res.z0)
    print("observation loss of the encoding", before, "after assimilation", after, "first fit loss", res.loss[0].cpu().numpy())
    assert (after < before).all(), (before, after)
    # the loss of the first iteration is the loss at the plain encoding
    assert np.allclose(res.loss[0].cpu().numpy(), before, rtol=1e-2)
    # a conditional encoder cannot be asked to fit param through assimilate
    from lns_amd._lib import LnsError
    cargs = tr.engine_args("E6")
    cargs.cond_encoder = True
    with pytest.raises(LnsError, match="conditional"):
        from lns_amd import dropin
        cm = dropin.build_dynamics(cargs)
        cm.assimilate(torch.zeros(1, cargs.in_channels, cargs.Ly, cargs.Lx), torch.zeros(1, 1, cargs.in_channels, cargs.Ly, cargs.Lx), [0],
                      torch.zeros(1), fit_param=True)

"""GPU: lns_train_backward_ex -- the state-only adjoint of the training rollout and the gradient with respect to `param`.

  * the state-only call (no gradient array) returns the bits of the full call's grad_z_in under both weight-gradient forms:
    the data path is the same kernels in the same order;
  * it writes no parameter gradient anywhere: buffers the full call filled are NaN-filled afterwards, are not passed, and stay
    NaN (nothing reaches them through pointers a previous call left behind);
  * it accepts a workspace that covers the layout without the partial-sum area of "train_wgrad" = 1, which the full call refuses;
  * grad_param of the conditional engines against the float64 statement (tests/latent_fit_reference.py: adjoint_reference)
    within max(GRAD_TOL, 3 x own) in rel-L2 and in max |diff| / max |ref| -- train_reference.bounds' rule -- in both modes and
    under both forms, at T = 1 and T >= 2; grad_z0 by the same rule;
  * `model(z_in, z_out, param.requires_grad_(), loss_fn)` fills param.grad with the C call's bits; a param that does not
    require grad keeps grad None.

Cases: the T = 1 / T >= 2, B = 1 / 33, one-row, 2x2 and 7x15 planes of the training-gradient grid, plain and conditional."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import latent_fit_reference as lf
import train_reference as tr

pytestmark = pytest.mark.gpu


def _need_gpu():
    assert torch.cuda.is_available(), "GPU test selected but no GPU is visible"


def test_latent_fit_is_built():
    """Fails on the parent: the symbols and the feature name."""
    from lns_amd import _lib
    L = _lib.lib()
    for s in ("lns_train_backward_ex", "lns_loss_obs_mse", "lns_fit_step", "lns_fit_step_workspace_bytes"):
        assert hasattr(L, s), s
    assert L.lns_build_has(b"latent_fit") == 1


def _setup(case, form):
    name, B, T, h, w = case
    model = tr.grid_model(name)
    eng = model._owner._eng
    eng.set_option("train_wgrad", form)
    _, z_in, z_out, prm = tr.case_inputs(case)
    params = {k: p.detach() for k, p in model.named_parameters() if k.startswith("propagator.")}
    z0 = torch.from_numpy(z_in[:, 0].copy()).cuda()
    zo = torch.from_numpy(z_out).cuda()
    p = torch.from_numpy(prm).cuda() if prm is not None else None
    z_pred, ws = eng.train_forward(params, z0, T, param=p)
    zp = z_pred.detach().clone().requires_grad_(True)
    F.smooth_l1_loss(zp, zo).backward()
    return model, eng, params, z0, zo, p, z_pred, ws, zp.grad.contiguous()


@pytest.mark.parametrize("form", tr.FORMS)
@pytest.mark.parametrize("case", lf.ADJOINT_CASES, ids=tr.case_id)
def test_state_only_adjoint(case, form):
    _need_gpu()
    from lns_amd import _lib
    name, B, T, h, w = case
    model, eng, params, z0, zo, p, z_pred, ws, g = _setup(case, form)
    cond = p is not None
    L = eng._L
    grads = {k: torch.empty_like(v) for k, v in params.items()}
    gz_full, gz_so = torch.empty_like(z0), torch.full_like(z0, float("nan"))
    gp_full = torch.empty(B, device="cuda") if cond else None
    gp_so = torch.full((B,), float("nan"), device="cuda") if cond else None
    stream = eng._stream(z0)

    def call(grads_arr, gz, gp, nbytes=ws.numel()):
        return L.lns_train_backward_ex(eng._h, eng._ptr_array(params), z0.data_ptr(), z_pred.data_ptr(), g.data_ptr(), B, h, w, T,
                                       grads_arr, gz.data_ptr(), ws.data_ptr(), nbytes, stream, gp.data_ptr() if gp is not None else None)
    assert call(eng._ptr_array(grads), gz_full, gp_full) == 0, L.lns_last_error(eng._h)
    torch.cuda.synchronize()
    assert all(torch.isfinite(t).all() for t in grads.values())
    for t in grads.values():
        t.fill_(float("nan"))
    # the smallest workspace the state-only adjoint needs: the layout without the partial-sum area
    eng.set_option("train_wgrad", 0)
    n0 = ctypes.c_size_t(0)
    assert L.lns_train_workspace_bytes(eng._h, B, h, w, T, ctypes.byref(n0)) == 0
    eng.set_option("train_wgrad", form)
    assert n0.value <= ws.numel()
    assert call(None, gz_so, gp_so, nbytes=n0.value) == 0, L.lns_last_error(eng._h)
    torch.cuda.synchronize()
    assert torch.equal(gz_so, gz_full)
    assert all(torch.isnan(t).all() for t in grads.values())
    if form == 1 and n0.value < ws.numel():
        assert call(eng._ptr_array(grads), gz_full, gp_full, nbytes=n0.value) == _lib.LNS_ENOMEM
    if not cond:
        gp = torch.empty(B, device="cuda")
        assert call(None, gz_so, gp) == _lib.LNS_EINVAL and "grad_param" in L.lns_last_error(eng._h).decode()
        r64, r32 = lf.adjoint_truth(case)
        e2, b2, em, bm, o2, om = lf.rule(gz_so.cpu().numpy(), r64["grad_z0"], r32["grad_z0"])
        assert e2 <= b2 and em <= bm, ("grad_z0", e2, b2, em, bm)
        return
    assert torch.equal(gp_so, gp_full)
    r64, r32 = lf.adjoint_truth(case)
    for ours, k in ((gz_so, "grad_z0"), (gp_so, "grad_param"), (gp_full, "grad_param")):
        e2, b2, em, bm, o2, om = lf.rule(ours.cpu().numpy(), r64[k], r32[k])
        print("%s form %d %s: rel-L2 %.2e/%.2e rel-max %.2e/%.2e (own %.2e %.2e)" % (tr.case_id(case), form, k, e2, b2, em, bm, o2, om))
        assert e2 <= b2, (k, "rel-L2", e2, b2, o2)
        assert em <= bm, (k, "rel-max", em, bm, om)


@pytest.mark.parametrize("case", [("E6", 5, 2, 7, 15), ("E6", 1, 1, 7, 15)], ids=tr.case_id)
def test_param_grad_arrives_through_autograd(case):
    _need_gpu()
    name, B, T, h, w = case
    model, eng, params, z0, zo, p, z_pred, ws, g = _setup(case, 0)
    _, _, gp = eng.train_backward(params, z0, z_pred, g, ws, need_z_grad=True, need_param_grad=True)
    zi = z0[:, None].clone()
    pr = p.clone().requires_grad_(True)
    for q in model.propagator.parameters():
        q.grad = None
    model(zi, zo, pr, F.smooth_l1_loss).backward()
    assert pr.grad is not None and pr.grad.shape == pr.shape and torch.equal(pr.grad, gp)
    weight_grads = {k: q.grad.clone() for k, q in model.named_parameters() if k.startswith("propagator.")}
    # without requires_grad nothing changes: no gradient for param, the same weight gradients
    for q in model.propagator.parameters():
        q.grad = None
    plain = p.clone()
    model(zi, zo, plain, F.smooth_l1_loss).backward()
    assert plain.grad is None
    for k, q in model.named_parameters():
        if k.startswith("propagator."):
            assert torch.equal(q.grad, weight_grads[k]), k

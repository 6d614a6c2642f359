"""GPU: the device-resident stage-2 training step (include/lns.h "device-resident training step"): the smooth-L1 and Adam
kernels against float64 numpy, the whole step against the autograd path + torch.optim.Adam and against the committed
gradient fixtures, optimiser-state hand-over with torch, no allocation inside the step, inference after training."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import GOLDEN, ROOT, rel_l2

pytestmark = pytest.mark.gpu

GRAD_CASES = ["ns2d_mini", "twophase", "sw_half_periodic", "twophase_cond"]      # as tests/test_gpu_parity.py
GRAD_TOL = 1e-4                                                                   # as tests/test_gpu_parity.py
STEP_CASES = ["ns2d_mini", "twophase_cond"]
LR = 5e-4


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _grad_meta(case):
    g = np.load(os.path.join(GOLDEN, "grads_%s.npz" % case))
    return g, json.loads(bytes(g["meta"]).decode())


def _ulp_err(got32, ref64):
    """Largest distance of got (fp32) from ref (float64) in units of the fp32 spacing at ref."""
    ref32 = ref64.astype(np.float32)
    sp = np.maximum(np.spacing(np.abs(ref32)).astype(np.float64), np.finfo(np.float32).tiny)
    return float((np.abs(got32.astype(np.float64) - ref64) / sp).max())


# ---- loss kernel -----------------------------------------------------------------------------------------------------
def _loss_sizes():
    out = []
    for case in GRAD_CASES:
        _, meta = _grad_meta(case)
        c, h, w = meta["latent"]
        out.append((case, meta["B"] * meta["T"] * c * h * w))
    return out + [("n1", 1), ("n3", 3), ("n4097", 4097), ("ns2d_shipped", 32 * 2 * 16 * 8 * 8), ("sw_shipped", 32 * 5 * 64 * 12 * 24)]


@pytest.mark.parametrize("beta", [0.25, 1.0])
@pytest.mark.parametrize("name,n", _loss_sizes())
def test_smooth_l1_kernel_matches_float64(name, n, beta):
    """lns_loss_smooth_l1 against the formula in float64 on the same fp32 inputs.  Loss: 1e-6 relative; gradient: 2 ulp per
    element; bit-identical run to run; torch's F.smooth_l1_loss + autograd as a second witness (loss 1e-6, gradient 4 ulp)."""
    _need_gpu()
    from lns_amd import engine
    rng = np.random.default_rng(1234 + n)
    pred = (rng.standard_normal(n) * 0.8 * beta).astype(np.float32)
    target = (rng.standard_normal(n) * 0.8 * beta).astype(np.float32)
    d = pred.astype(np.float64) - target.astype(np.float64)
    inside = np.abs(d) < beta
    if n >= 1000:                       # |d| straddles beta: at least 10 % of the elements on each side (checkable without a GPU)
        assert 0.1 <= inside.mean() <= 0.9, inside.mean()
    loss64 = np.where(inside, 0.5 * d * d / beta, np.abs(d) - 0.5 * beta).mean()
    grad64 = np.where(inside, d / beta, np.sign(d)) / n
    p, t = torch.from_numpy(pred).cuda(), torch.from_numpy(target).cuda()
    loss, grad = engine.smooth_l1(p, t, beta=beta)
    loss2, grad2 = engine.smooth_l1(p, t, beta=beta)
    only_loss, none = engine.smooth_l1(p, t, beta=beta, need_grad=False)
    torch.cuda.synchronize()
    l_rel = abs(float(loss.item()) - loss64) / abs(loss64)
    g_ulp = _ulp_err(grad.cpu().numpy(), grad64)
    print("smooth_l1 %s n=%d beta=%g: loss rel err %.3e, gradient worst %.2f ulp" % (name, n, beta, l_rel, g_ulp))
    assert l_rel <= 1e-6, (l_rel, loss.item(), loss64)
    assert g_ulp <= 2.0, g_ulp
    assert torch.equal(loss.view(torch.int32), loss2.view(torch.int32)) and torch.equal(grad.view(torch.int32), grad2.view(torch.int32))
    assert none is None and torch.equal(only_loss.view(torch.int32), loss.view(torch.int32))
    # second witness
    pt = p.clone().requires_grad_(True)
    lt = F.smooth_l1_loss(pt, t, beta=beta)
    lt.backward()
    assert abs(float(lt.item()) - float(loss.item())) <= 1e-6 * abs(loss64), (lt.item(), loss.item())
    t_ulp = _ulp_err(grad.cpu().numpy(), pt.grad.cpu().numpy().astype(np.float64))
    assert t_ulp <= 4.0, t_ulp


def test_smooth_l1_handles_unaligned_views_with_the_same_bits():
    """Pointers that are not 16-byte aligned take the scalar path: same elements per thread, same order, same bits."""
    _need_gpu()
    from lns_amd import engine
    n = 3 * 4096 + 5
    gen = torch.Generator(device="cuda").manual_seed(5)
    buf_p = torch.randn(n + 1, device="cuda", generator=gen)
    buf_t = torch.randn(n + 1, device="cuda", generator=gen)
    la, ga = engine.smooth_l1(buf_p[1:], buf_t[1:], beta=0.5)                      # 4-byte offset views
    lb, gb = engine.smooth_l1(buf_p[1:].clone(), buf_t[1:].clone(), beta=0.5)      # aligned copies
    torch.cuda.synchronize()
    assert torch.equal(la.view(torch.int32), lb.view(torch.int32)) and torch.equal(ga.view(torch.int32), gb.view(torch.int32))


# ---- Adam kernel -----------------------------------------------------------------------------------------------------
ADAM_SIZES = (1, 7, 128, 4099, 147456)
# |p - p64| <= ADAM_REL |p64| + ADAM_ABS_LR lr: a few fp32 roundings of the parameter (6e-8 each) and of the update, whose
# magnitude is at most ~3 lr per step and whose relative error is ~1e-6, over 10 steps.  Derived, not fitted.
ADAM_REL, ADAM_ABS_LR = 4e-7, 2e-5
MOMENT_REL = 1e-6


def _adam64(p, g, m, v, t, lr, b1, b2, eps, wd):
    g = g + wd * p
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    p = p - (lr / (1 - b1 ** t)) * m / (np.sqrt(v) / np.sqrt(1 - b2 ** t) + eps)
    return p, m, v


@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_adam_kernel_matches_float64(wd):
    """lns_adam_step_tensors, five tensors from 1 to 147 456 elements in ONE call (chunk boundaries, tails, tiny tensors)
    plus an entry without a gradient, 10 steps with fresh gradients, against a float64 numpy Adam started from the same fp32
    state; torch.optim.Adam(foreach=False) on the GPU is held to the same bound as a yardstick."""
    _need_gpu()
    from lns_amd import _lib, engine
    L = _lib.lib()
    b1, b2, eps = 0.9, 0.999, 1e-8
    rng = np.random.default_rng(7)
    p0 = [rng.standard_normal(n).astype(np.float32) * np.float32(0.3) for n in ADAM_SIZES]
    dev = torch.device("cuda", 0)
    P = [torch.from_numpy(a.copy()).to(dev) for a in p0]
    M = [torch.zeros_like(a) for a in P]
    V = [torch.zeros_like(a) for a in P]
    G = [torch.zeros_like(a) for a in P]
    skipped = torch.from_numpy(rng.standard_normal(300).astype(np.float32)).to(dev)       # all pointers but the gradient
    skipped0 = skipped.clone()
    sk_m, sk_v = torch.ones(300, device=dev), torch.ones(300, device=dev)
    tp = [torch.nn.Parameter(torch.from_numpy(a.copy()).to(dev)) for a in p0]
    topt = torch.optim.Adam(tp, lr=LR, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
    p64 = [a.astype(np.float64) for a in p0]
    m64 = [np.zeros_like(a) for a in p64]
    v64 = [np.zeros_like(a) for a in p64]
    n = len(P) + 1
    vp = ctypes.c_void_p * n
    numel = (ctypes.c_int64 * n)(*[a.numel() for a in P], 300)
    worst = dict(ours=0.0, torch=0.0, m=0.0, v=0.0, torch_m=0.0, torch_v=0.0)

    def rel(got, ref):                                   # per tensor: largest error relative to the tensor's largest entry
        return float(np.abs(got.detach().cpu().numpy().astype(np.float64) - ref).max() / np.abs(ref).max())
    for t in range(1, 11):
        gs = [rng.standard_normal(a.size).astype(np.float32) * np.float32(0.05) for a in p0]
        for i, g in enumerate(gs):
            G[i].copy_(torch.from_numpy(g))
            tp[i].grad = torch.from_numpy(g).to(dev)
        spec = engine.adam_spec(LR, (b1, b2), eps, wd, step=t)
        rc = L.lns_adam_step_tensors(n, vp(*[a.data_ptr() for a in P], skipped.data_ptr()), vp(*[a.data_ptr() for a in G], None),
                                     vp(*[a.data_ptr() for a in M], sk_m.data_ptr()), vp(*[a.data_ptr() for a in V], sk_v.data_ptr()),
                                     numel, ctypes.byref(spec), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, L.lns_create_error()
        topt.step()
        torch.cuda.synchronize()
        for i, g in enumerate(gs):
            g64 = g.astype(np.float64)
            p64[i], m64[i], v64[i] = _adam64(p64[i], g64, m64[i], v64[i], t, LR, b1, b2, eps, wd)
            bound = ADAM_REL * np.abs(p64[i]) + ADAM_ABS_LR * LR
            ours = np.abs(P[i].cpu().numpy().astype(np.float64) - p64[i]) / bound
            theirs = np.abs(tp[i].detach().cpu().numpy().astype(np.float64) - p64[i]) / bound
            worst["ours"], worst["torch"] = max(worst["ours"], ours.max()), max(worst["torch"], theirs.max())
            # the moments: plain per-tensor relative error, torch's own moments held to the same measure
            st = topt.state[tp[i]]
            worst["m"], worst["v"] = max(worst["m"], rel(M[i], m64[i])), max(worst["v"], rel(V[i], v64[i]))
            worst["torch_m"] = max(worst["torch_m"], rel(st["exp_avg"], m64[i]))
            worst["torch_v"] = max(worst["torch_v"], rel(st["exp_avg_sq"], v64[i]))
    print("adam wd=%g: worst error / bound: ours %.3f, torch foreach=False %.3f; exp_avg rel %.2e (torch %.2e), exp_avg_sq rel %.2e "
          "(torch %.2e)" % (wd, worst["ours"], worst["torch"], worst["m"], worst["torch_m"], worst["v"], worst["torch_v"]))
    assert worst["torch"] <= 1.0, "the yardstick itself misses the derived bound: %r" % (worst,)
    assert worst["ours"] <= 1.0, worst
    assert worst["torch_m"] <= MOMENT_REL and worst["torch_v"] <= MOMENT_REL, "the yardstick itself misses 1e-6: %r" % (worst,)
    assert worst["m"] <= MOMENT_REL and worst["v"] <= MOMENT_REL, worst
    assert torch.equal(skipped.view(torch.int32), skipped0.view(torch.int32))             # null gradient: bits untouched
    assert bool((sk_m == 1).all()) and bool((sk_v == 1).all())


def test_adam_optimizer_on_the_engine_table_and_more_than_one_launch():
    """Engine.adam_step (lns_adam_step, lengths from the parameter table) and lns_amd.optim.Adam over more tensors than one
    kernel-argument block holds (96), against torch.optim.Adam."""
    _need_gpu()
    from lns_amd import config, dropin, optim
    gen = torch.Generator(device="cuda").manual_seed(3)
    ours = [torch.nn.Parameter(torch.randn(1 + 37 * (i % 11), device="cuda", generator=gen)) for i in range(130)]
    theirs = [torch.nn.Parameter(p.detach().clone()) for p in ours]
    oa = optim.Adam(ours, lr=LR, weight_decay=1e-2)
    ta = torch.optim.Adam(theirs, lr=LR, weight_decay=1e-2, foreach=False)
    for _ in range(3):
        for p, q in zip(ours, theirs):
            p.grad = torch.randn(p.shape, device="cuda", generator=gen)
            q.grad = p.grad.clone()
        v0 = ours[0]._version
        oa.step()
        ta.step()
        assert ours[0]._version > v0
    for p, q in zip(ours, theirs):
        assert float((p - q).abs().max()) <= ADAM_REL * float(q.abs().max()) + ADAM_ABS_LR * LR
    # the engine-table form: every propagator tensor of a model
    m = dropin.build_dynamics(config.preset("ns2d_mini")).cuda()
    names = [k for k, _ in m.named_parameters() if k.startswith("propagator.")]
    named = dict(m.named_parameters())
    prm = {k: named[k].detach() for k in names}
    ref = {k: torch.nn.Parameter(prm[k].clone()) for k in names}
    grads = {k: torch.randn(prm[k].shape, device="cuda", generator=gen) for k in names}
    ea = {k: torch.zeros_like(prm[k]) for k in names}
    es = {k: torch.zeros_like(prm[k]) for k in names}
    untouched = names[3]
    part = {k: v for k, v in grads.items() if k != untouched}
    before = prm[untouched].clone()
    m._eng.adam_step(prm, part, ea, es, lr=LR, step=1)
    ta = torch.optim.Adam(list(ref.values()), lr=LR, foreach=False)
    for k in names:
        ref[k].grad = grads[k]
    ta.step()
    torch.cuda.synchronize()
    assert torch.equal(prm[untouched], before)
    for k in names:
        if k != untouched:
            assert float((prm[k] - ref[k]).abs().max()) <= ADAM_REL * float(ref[k].abs().max()) + ADAM_ABS_LR * LR, k


# ---- the whole step --------------------------------------------------------------------------------------------------
def _setup(case, reverse=False):
    import gpu_checks as gc
    from lns_amd import config, filler
    g, meta = _grad_meta(case)
    args = config.preset(meta["preset"])
    model, _ = gc.build_models(args, meta["weight_seed"])
    B, T = meta["B"], meta["T"]
    c, h, w = meta["latent"]
    z_in = torch.from_numpy(filler.normal("z_in", (B, 1, c, h, w), meta["input_seed"]) * np.float32(meta["z_scale"])).cuda()
    z_out = torch.from_numpy(filler.normal("z_out", (B, T, c, h, w), meta["input_seed"]) * np.float32(meta["z_scale"])).cuda()
    prm = None
    if args.family == "twophase_cond":
        prm = torch.from_numpy(filler.uniform01("param", B, meta["input_seed"]).astype(np.float32)).cuda()
    if reverse:
        z_in, z_out = z_in.flip(0).contiguous(), z_out.flip(0).contiguous()
        prm = prm.flip(0).contiguous() if prm is not None else None
    for p_ in model._ae.parameters():
        p_.requires_grad_(False)
    return g, meta, model, z_in, z_out, prm


def _prop(model):
    return {k: p for k, p in model.named_parameters() if k.startswith("propagator.")}


def _autograd_steps(model, z_in, z_out, prm, K, opt=None):
    """K steps of the existing path: model(z_in, z_out[, param], F.smooth_l1_loss); loss.backward(); Adam.step()."""
    opt = opt or torch.optim.Adam(model.propagator.parameters(), lr=LR)
    losses, first_grads, traj = [], None, []
    for _ in range(K):
        opt.zero_grad()
        loss = model(z_in, z_out, *((prm,) if prm is not None else ()), F.smooth_l1_loss)
        loss.backward()
        if first_grads is None:
            first_grads = {k: p.grad.detach().clone() for k, p in _prop(model).items()}
        opt.step()
        losses.append(loss.item())
        traj.append({k: p.detach().clone() for k, p in _prop(model).items()})
    return losses, first_grads, traj


@pytest.mark.parametrize("case", STEP_CASES)
def test_step_gradients_pass_the_reference_fixture(case):
    """Gradients produced by lns_train_step with adam_spec = NULL (Stage2Trainer.step(update=False)) under the comparison
    of tests/test_gpu_parity.py::test_training_rollout_gradients_match_reference: same fixtures, same GRAD_TOL, same
    `3 x own` rule."""
    _need_gpu()
    from lns_amd import train
    g, meta, model, z_in, z_out, prm = _setup(case)
    before = {k: p.detach().clone() for k, p in _prop(model).items()}
    tr = train.Stage2Trainer(model, lr=LR)
    loss = tr.step(z_in, z_out, prm, update=False)
    torch.cuda.synchronize()
    assert abs(loss.item() - float(g["loss"])) <= 2e-6 * abs(float(g["loss"])) + 1e-7, (loss.item(), float(g["loss"]))
    params = dict(model.named_parameters())
    sub = meta["sub"]
    for k in meta["keys"]:
        gr = params[k].grad
        assert gr is not None and torch.isfinite(gr).all(), k
        gh = gr.detach().cpu().numpy().astype(np.float64).ravel()
        ref32, ref64 = g["gsub:" + k].astype(np.float64), g["gsub_f64:" + k].astype(np.float64)
        own = rel_l2(ref32, ref64)
        e32, e64 = rel_l2(gh[::sub], ref32), rel_l2(gh[::sub], ref64)
        en = abs(np.sqrt((gh ** 2).sum()) / float(g["gnorm_f64:" + k]) - 1.0)
        assert e64 <= max(GRAD_TOL, 3.0 * own), (k, e32, e64, own)
        assert e32 <= max(GRAD_TOL, 3.0 * own), (k, e32, e64, own)
        assert en <= max(GRAD_TOL, 3.0 * own), (k, en)
    for k, p in _prop(model).items():                                   # no update was asked for
        assert torch.equal(p.detach(), before[k]), k
    assert all(p_.grad is None for p_ in model._ae.parameters())


@pytest.mark.parametrize("case", STEP_CASES)
def test_step_matches_the_autograd_path(case):
    """Model A: K = 5 steps of (autograd path + torch.optim.Adam); model B: K Stage2Trainer.step on the same batch.
    Step 1 (before any update): loss within 2e-6 relative, every gradient within rel-L2 1e-5.  After K steps B's distance
    from A, relative to how far A moved, is gated at 3 x the path's own fp32 spread -- A re-run with its batch rows reversed
    (same mean loss, another summation order) -- with a floor of 1e-4.  The loss falls on the fixed batch for both."""
    _need_gpu()
    from lns_amd import train
    K = 5
    _, _, model_a, z_in, z_out, prm = _setup(case)
    init = {k: p.detach().clone() for k, p in _prop(model_a).items()}
    loss_a, grads_a, traj_a = _autograd_steps(model_a, z_in, z_out, prm, K)
    _, _, model_r, rz_in, rz_out, rprm = _setup(case, reverse=True)
    _, _, traj_r = _autograd_steps(model_r, rz_in, rz_out, rprm, K)
    _, _, model_b, _, _, _ = _setup(case)
    tr = train.Stage2Trainer(model_b, lr=LR)
    loss_b, traj_b, grads_b = [], [], None
    for _ in range(K):
        loss_b.append(tr.step(z_in, z_out, prm).clone())
        if grads_b is None:
            grads_b = {k: p.grad.detach().clone() for k, p in _prop(model_b).items()}
        traj_b.append({k: p.detach().clone() for k, p in _prop(model_b).items()})
    torch.cuda.synchronize()
    loss_b = [l.item() for l in loss_b]
    assert abs(loss_b[0] - loss_a[0]) <= 2e-6 * abs(loss_a[0]), (loss_b[0], loss_a[0])
    worst_g = max((rel_l2(grads_b[k].cpu().numpy(), grads_a[k].cpu().numpy()), k) for k in grads_a)
    assert worst_g[0] <= 1e-5, worst_g

    def spread(traj):
        out = {}
        for k in init:
            moved = [float((traj_a[i][k] - init[k]).norm()) for i in range(K)]
            out[k] = max(float((traj[i][k] - traj_a[i][k]).norm()) / moved[i] for i in range(K) if moved[i] > 0)
        return out
    own, ours = spread(traj_r), spread(traj_b)
    k_own, k_ours = max(own, key=own.get), max(ours, key=ours.get)
    record = dict(case=case, K=K, lr=LR, own_spread_max=own[k_own], own_spread_tensor=k_own, trainer_vs_autograd_max=ours[k_ours],
                  trainer_vs_autograd_tensor=k_ours, step1_loss_rel=abs(loss_b[0] - loss_a[0]) / abs(loss_a[0]),
                  step1_grad_rel_l2_max=worst_g[0], loss_autograd=loss_a, loss_trainer=loss_b)
    print("train_step_parity", json.dumps(record))
    if os.environ.get("LNS_WRITE_PROFILES"):                # the committed record (profiles/train_step_parity.json) is written on request only
        path = os.path.join(ROOT, "profiles", "train_step_parity.json")
        allr = json.load(open(path)) if os.path.exists(path) else {}
        allr[case] = record
        with open(path, "w") as f:
            json.dump(allr, f, indent=1, sort_keys=True)
    for k in init:
        assert ours[k] <= max(1e-4, 3.0 * own[k]), (k, ours[k], own[k])
    assert loss_a[-1] < loss_a[0] and loss_b[-1] < loss_b[0], (loss_a, loss_b)


def _checkpointed(state_dict):
    """The state_dict as it comes back from an `optim_*.pt` file (train_stage2_ns2d.py:203).  `load_state_dict` itself keeps
    the tensors it is given (no copy when dtype and device already match), so handing one live optimiser's state_dict to
    another would make the two share their moments and step counters."""
    import io
    f = io.BytesIO()
    torch.save(state_dict, f)
    f.seek(0)
    return torch.load(f)


def test_optimizer_state_moves_between_torch_and_the_trainer():
    """After 3 trainer steps optimizer.state_dict() loads into a torch.optim.Adam over clones of the parameters; one more step
    on both sides from the same gradients agrees within the Adam bound.  And the reverse: torch state -> lns_amd.optim.Adam."""
    _need_gpu()
    from lns_amd import optim, train
    _, _, model, z_in, z_out, _ = _setup("ns2d_mini")
    tr = train.Stage2Trainer(model, lr=LR, weight_decay=1e-2)
    for _ in range(3):
        tr.step(z_in, z_out)
    prop = list(model.propagator.parameters())
    clones = [torch.nn.Parameter(p.detach().clone()) for p in prop]
    topt = torch.optim.Adam(clones, lr=1.0, foreach=False)
    topt.load_state_dict(_checkpointed(tr.optimizer.state_dict()))
    assert topt.param_groups[0]["lr"] == LR and topt.param_groups[0]["weight_decay"] == 1e-2
    assert all(float(topt.state[c]["step"]) == 3.0 for c in clones)
    tr.step(z_in, z_out, update=False)                                   # this step's gradients, parameters untouched
    for c, p in zip(clones, prop):
        c.grad = p.grad.detach().clone()
    tr.optimizer.step()                                                  # the one-launch kernel on p.grad
    topt.step()
    torch.cuda.synchronize()

    def close(ps, qs):
        for p, q in zip(ps, qs):
            tol = ADAM_REL * q.detach().abs() + ADAM_ABS_LR * LR
            assert bool(((p.detach() - q.detach()).abs() <= tol).all())
    close(prop, clones)
    assert all(float(tr.optimizer.state[p]["step"]) == 4.0 for p in prop) and all(float(topt.state[c]["step"]) == 4.0 for c in clones)
    # reverse: the torch optimiser's state (4 steps) -> a fresh lns Adam over a third copy; the trainer keeps working on it
    third = [torch.nn.Parameter(c.detach().clone()) for c in clones]
    back = optim.Adam(third, lr=123.0)
    back.load_state_dict(_checkpointed(topt.state_dict()))
    gen = torch.Generator(device="cuda").manual_seed(9)
    for c, q in zip(clones, third):
        c.grad = torch.randn(c.shape, device="cuda", generator=gen) * 0.01
        q.grad = c.grad.clone()
    topt.step()
    back.step()
    torch.cuda.synchronize()
    close(third, clones)
    assert all(float(back.state[q]["step"]) == 5.0 for q in third)
    # and the trainer resolves a loaded state: its next step uses the loaded moments (step count 5 -> 6)
    tr.optimizer.load_state_dict(_checkpointed(topt.state_dict()))
    tr.step(z_in, z_out)
    assert all(float(tr.optimizer.state[p]["step"]) == 6.0 for p in prop)


def test_no_hidden_work_in_the_step():
    """After two warm-up steps, 20 steps allocate nothing; .grad keeps its storage; the autoencoder is untouched; a replaced
    Parameter object is picked up."""
    _need_gpu()
    from lns_amd import train
    _, _, model, z_in, z_out, _ = _setup("ns2d_mini")
    tr = train.Stage2Trainer(model, lr=LR)
    ae_before = {k: p.detach().clone() for k, p in model._ae.named_parameters()}
    for _ in range(2):
        tr.step(z_in, z_out)
    torch.cuda.synchronize()
    prop = _prop(model)
    ptrs = {k: p.grad.data_ptr() for k, p in prop.items()}
    n0 = torch.cuda.memory_stats()["allocation.all.allocated"]
    for _ in range(20):
        loss = tr.step(z_in, z_out)
    n1 = torch.cuda.memory_stats()["allocation.all.allocated"]
    torch.cuda.synchronize()
    assert n1 == n0, (n0, n1)
    assert np.isfinite(loss.item())
    assert all(p.grad.data_ptr() == ptrs[k] for k, p in prop.items())
    for k, p in model._ae.named_parameters():
        assert p.grad is None and torch.equal(p.detach(), ae_before[k]), k
    # zero_grad(set_to_none=True) between steps: the buffers come back
    tr.optimizer.zero_grad(set_to_none=True)
    tr.step(z_in, z_out)
    assert all(p.grad is not None and p.grad.data_ptr() == ptrs[k] for k, p in prop.items())
    # a replaced Parameter object: the next step updates the new tensor, not the old storage
    old = model.propagator.in_proj.weight
    old_val = old.detach().clone()
    new = torch.nn.Parameter(old.detach().clone() * 1.01)
    new_val = new.detach().clone()
    model.propagator.in_proj.weight = new
    tr.step(z_in, z_out)
    torch.cuda.synchronize()
    assert torch.equal(old.detach(), old_val)
    assert not torch.equal(new.detach(), new_val)
    assert new.grad is not None and any(p is new for p in tr.optimizer.param_groups[0]["params"])
    assert float(tr.optimizer.state[new]["step"]) == float(tr.optimizer.state[getattr(model.propagator.out_proj, "1").weight]["step"])


def test_inference_sees_the_trained_weights():
    """model.predict after trainer steps = predict of a fresh model loaded from the trained state_dict, bit for bit: the
    in-place kernel updates bump what _weights_signature watches."""
    _need_gpu()
    import gpu_checks as gc
    from lns_amd import config, filler, train
    _, meta, model, z_in, z_out, _ = _setup("ns2d_mini")
    args = config.preset(meta["preset"])
    x = torch.from_numpy(filler.normal("x", (2, args.in_channels, args.Ly, args.Lx), 7)).cuda()
    y0 = model.predict(x, 3, to_x=True).clone()                         # weights resident in the inference engine
    tr = train.Stage2Trainer(model, lr=1e-2)
    v0 = model.propagator.in_proj.weight._version
    for _ in range(3):
        tr.step(z_in, z_out)
    assert model.propagator.in_proj.weight._version >= v0 + 3
    y1 = model.predict(x, 3, to_x=True)
    fresh, _ = gc.build_models(args, meta["weight_seed"] + 1)
    fresh.load_state_dict(model.state_dict())
    y2 = fresh.predict(x, 3, to_x=True)
    torch.cuda.synchronize()
    assert not torch.equal(y1, y0)
    assert torch.equal(y1.view(torch.int32), y2.view(torch.int32))

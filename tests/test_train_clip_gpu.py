"""GPU: gradient-norm clipping, AdamW and skip_nonfinite of the device-resident training step (include/lns.h
"gradient-norm clipping and AdamW"): the norm kernels against float64, AdamW against torch.optim.AdamW, the clipped
Stage2Trainer against the unfused sequence (step(update=False), torch.nn.utils.clip_grad_norm_, optim.Adam.step()), and
the plain trainer untouched."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

LR = 5e-4                                  # as tests/test_train_step_gpu.py
# tests/test_train_step_gpu.py:105 (applied to lns_amd.optim.Adam against torch.optim.Adam at :201): |p - q| <=
# ADAM_REL max|q| + ADAM_ABS_LR lr per tensor
ADAM_REL, ADAM_ABS_LR = 4e-7, 2e-5
NORM_REL = 2.4e-7                          # 2 ulp of fp32: squares of fp32 values are exact in double, the chain is double
STEP_CASES = ["ns2d_mini", "twophase_cond"]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ulp_err(got32, ref64):
    """Largest distance of got (fp32) from ref (float64) in units of the fp32 spacing at ref."""
    ref32 = ref64.astype(np.float32)
    sp = np.maximum(np.spacing(np.abs(ref32)).astype(np.float64), np.finfo(np.float32).tiny)
    return float((np.abs(got32.astype(np.float64) - ref64) / sp).max())


def _norm_call(tensors, max_norm, flags=0, counter=None):
    """lns_grad_norm_tensors on a list of device tensors -> (norm, coef) as numpy fp32 scalars (synchronises)."""
    from lns_amd import _lib
    L = _lib.lib()
    n = len(tensors)
    ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in tensors])
    numel = (ctypes.c_int64 * n)(*[t.numel() for t in tensors])
    nb = ctypes.c_size_t(0)
    assert L.lns_grad_norm_scratch_bytes(n, numel, ctypes.byref(nb)) == 0
    scratch = torch.empty(nb.value, dtype=torch.uint8, device="cuda")
    out = torch.full((2,), -7.0, device="cuda")
    rc = L.lns_grad_norm_tensors(n, ptrs, numel, float(max_norm), out.data_ptr(), out.data_ptr() + 4,
                                 counter.data_ptr() if counter is not None else None, flags, scratch.data_ptr(), nb.value, _stream())
    assert rc == 0, L.lns_create_error()
    o = out.cpu().numpy()
    return o[0], o[1]


def _norm64(tensors):
    return float(np.sqrt(sum((t.detach().cpu().numpy().astype(np.float64) ** 2).sum() for t in tensors)))


def _coef64(norm32, max_norm):
    """clip_grad_norm_'s coefficient from the DEVICE's fp32 norm, in float64: the kernel's fp32 sum and quotient round
    once each, so it lies within 1 ulp of this."""
    return min(1.0, float(np.float32(max_norm)) / (float(norm32) + float(np.float32(1e-6))))


def _norm_lists():
    gen = torch.Generator(device="cuda").manual_seed(11)
    sizes = [1, 3, 2047, 2048, 2049, 5000]
    base = torch.randn(4097, device="cuda", generator=gen)
    mixed = [torch.randn(n, device="cuda", generator=gen) * (0.1 + i) for i, n in enumerate(sizes)] + [base[1:]]      # + one unaligned view
    assert mixed[-1].data_ptr() % 16 == 4 and mixed[-1].is_contiguous()
    many = [torch.randn(1 + 53 * (i % 7), device="cuda", generator=gen) for i in range(96)] + [torch.randn(2049, device="cuda", generator=gen) * 3]
    return dict(mixed=mixed, many97=many, single1=[mixed[0]], tail2049=[mixed[4]])


@pytest.mark.parametrize("which", ["mixed", "many97", "single1", "tail2049"])
def test_grad_norm_matches_float64_and_is_reproducible(which):
    """lns_grad_norm_tensors over tensors of 1 / 3 / 2047 / 2048 / 2049 / 5000 elements and a view at an offset of one float,
    and over 97 tensors (two launches: the table holds 96): the norm within 2 ulp of fp32 (2.4e-7) of the float64 norm,
    bit-identical between two calls, the coefficient within 1 ulp of min(1, max_norm / (norm + 1e-6)) for a max_norm below
    and one above the norm, exactly 1 for max_norm <= 0."""
    _need_gpu()
    ts = _norm_lists()[which]
    ref = _norm64(ts)
    for max_norm in (0.5 * ref, 2.0 * ref):
        norm, coef = _norm_call(ts, max_norm)
        norm2, coef2 = _norm_call(ts, max_norm)
        rel = abs(float(norm) - ref) / ref
        c64 = _coef64(norm, max_norm)
        c_ulp = _ulp_err(np.array([coef]), np.array([c64]))
        print("grad_norm %s max_norm=%.4g: norm %.9g (float64 %.12g, rel %.2e), coef %.9g (%.2f ulp)" % (which, max_norm, norm, ref, rel, coef, c_ulp))
        assert rel <= NORM_REL, (norm, ref, rel)
        assert norm.tobytes() == norm2.tobytes() and coef.tobytes() == coef2.tobytes()
        assert c_ulp <= 1.0, (coef, c64)
        assert (coef < 1.0) == (max_norm < ref)
    norm, coef = _norm_call(ts, 0.0)
    assert abs(float(norm) - ref) / ref <= NORM_REL and coef == 1.0
    # a positive max_norm below fp32's smallest denormal still clips (to ~0, as torch would): it is not "no clipping"
    _, coef = _norm_call(ts, 1e-60)
    assert 0.0 <= coef < 1e-30


def test_grad_norm_unaligned_view_has_the_bits_of_an_aligned_copy():
    """The scalar path visits the same elements in the same order as the 16-byte path."""
    _need_gpu()
    gen = torch.Generator(device="cuda").manual_seed(5)
    base = torch.randn(5001, device="cuda", generator=gen)
    view = base[1:]
    a, _ = _norm_call([view], 1.0)
    b, _ = _norm_call([view.clone()], 1.0)
    assert a.tobytes() == b.tobytes()


def test_grad_norm_skip_flag_and_counter():
    """An inf or NaN norm under LNS_UPDATE_SKIP_NONFINITE: coef = -1 and the counter moves; without the flag inf gives
    coef = 0 and NaN a NaN coef (torch's clamp keeps NaN), and the counter stays."""
    _need_gpu()
    from lns_amd import _lib
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    good = torch.ones(3000, device="cuda")
    for bad_value in (float("inf"), float("nan")):
        bad = good.clone()
        bad[2500] = bad_value
        norm, coef = _norm_call([good, bad], 1.0, flags=_lib.LNS_UPDATE_SKIP_NONFINITE, counter=counter)
        assert not np.isfinite(norm) and coef == -1.0
        norm, coef = _norm_call([good, bad], 1.0, flags=0, counter=counter)
        assert not np.isfinite(norm) and (coef == 0.0 if bad_value == float("inf") else np.isnan(coef))
    norm, coef = _norm_call([good], 1.0, flags=_lib.LNS_UPDATE_SKIP_NONFINITE, counter=counter)
    assert np.isfinite(norm) and 0.0 < coef < 1.0
    assert int(counter.item()) == 2


def test_clip_grad_norm_function_matches_torch():
    """lns_amd.optim.clip_grad_norm_ against torch.nn.utils.clip_grad_norm_ on cloned gradients: the returned norm (a device
    tensor) within 1e-6, the float64 norm the arbiter; the scaled gradients within 2 ulp of g * coef in float64."""
    _need_gpu()
    from lns_amd import optim
    gen = torch.Generator(device="cuda").manual_seed(2)
    ps = [torch.nn.Parameter(torch.zeros(n, device="cuda")) for n in (1, 77, 2049, 6000)]
    qs = [torch.nn.Parameter(torch.zeros(n, device="cuda")) for n in (1, 77, 2049, 6000)]
    for p, q in zip(ps, qs):
        p.grad = torch.randn(p.shape, device="cuda", generator=gen)
        q.grad = p.grad.clone()
    g0 = [p.grad.clone() for p in ps]
    ref = _norm64(g0)
    for max_norm in (0.25 * ref, 4.0 * ref):
        for p, q, g in zip(ps, qs, g0):
            p.grad.copy_(g)
            q.grad.copy_(g)
        ours = optim.clip_grad_norm_(ps, max_norm)
        theirs = torch.nn.utils.clip_grad_norm_(qs, max_norm, foreach=False)
        assert ours.dim() == 0 and ours.is_cuda
        o, t = float(ours.item()), float(theirs.item())
        assert abs(o - ref) / ref <= NORM_REL
        assert abs(o - t) / ref <= 1e-6 or abs(o - ref) <= abs(t - ref), (o, t, ref)
        c64 = _coef64(np.float32(o), max_norm)
        for p, g in zip(ps, g0):
            assert _ulp_err(p.grad.cpu().numpy(), g.cpu().numpy().astype(np.float64) * c64) <= 2.0


def test_adamw_matches_torch_adamw():
    """lns_amd.optim.AdamW against torch.optim.AdamW(foreach=False): five steps, weight_decay = 1e-2, sizes with a tail, more
    than one chunk and a parameter viewed at an offset of one float, under the tolerance tests/test_train_step_gpu.py:201
    applies to lns_amd.optim.Adam against torch.optim.Adam (ADAM_REL, ADAM_ABS_LR of its line 105)."""
    _need_gpu()
    from lns_amd import optim
    gen = torch.Generator(device="cuda").manual_seed(3)
    base = torch.randn(4100, device="cuda", generator=gen)
    ours = [torch.nn.Parameter(torch.randn(n, device="cuda", generator=gen)) for n in (1, 7, 2047, 2049, 5000)] + [torch.nn.Parameter(base[1:])]
    assert ours[-1].data_ptr() % 16 == 4
    theirs = [torch.nn.Parameter(p.detach().clone()) for p in ours]
    start = [p.detach().clone() for p in ours]
    oa = optim.AdamW(ours, lr=LR, weight_decay=1e-2)
    ta = torch.optim.AdamW(theirs, lr=LR, weight_decay=1e-2, foreach=False)
    l2 = [torch.nn.Parameter(p.detach().clone()) for p in ours]
    la = optim.Adam(l2, lr=LR, weight_decay=1e-2)                       # the L2 form: must NOT be what AdamW computes
    for _ in range(5):
        for p, q, r in zip(ours, theirs, l2):
            p.grad = torch.randn(p.shape, device="cuda", generator=gen)
            q.grad = p.grad.clone()
            r.grad = p.grad.clone()
        g_before = [p.grad.clone() for p in ours]
        v0 = ours[0]._version
        oa.step()
        ta.step()
        la.step()
        assert ours[0]._version > v0
        assert all(torch.equal(p.grad, g) for p, g in zip(ours, g_before))          # no coefficient: gradients stay
    worst = 0.0
    for p, q in zip(ours, theirs):
        tol = ADAM_REL * float(q.detach().abs().max()) + ADAM_ABS_LR * LR
        worst = max(worst, float((p - q).detach().abs().max()) / tol)
        assert float((p - q).detach().abs().max()) <= tol
    print("adamw vs torch.optim.AdamW: worst error / bound %.3f" % worst)
    assert all(float(oa.state[p]["step"]) == 5.0 for p in ours)
    assert any(float((p - r).detach().abs().max()) > 10 * (ADAM_REL * float(r.detach().abs().max()) + ADAM_ABS_LR * LR) for p, r in zip(ours[3:], l2[3:]))
    assert all(not torch.equal(p.detach(), s) for p, s in zip(ours, start))


# ---- the trainer -----------------------------------------------------------------------------------------------------
BATCH = {"ns2d_mini": (4, 2), "twophase_cond": (2, 2)}          # (B, T) of the trainer tests


def _setup(case, reverse=False):
    """As tests/test_train_step_gpu.py::_setup -- the model, latent size, seeds and scale of the committed gradient fixture --
    with the batch cut to BATCH[case]."""
    import gpu_checks as gc
    from lns_amd import config, filler
    g = np.load(os.path.join(GOLDEN, "grads_%s.npz" % case))
    meta = json.loads(bytes(g["meta"]).decode())
    args = config.preset(meta["preset"])
    model, _ = gc.build_models(args, meta["weight_seed"])
    B, T = BATCH[case]
    c, h, w = model._eng.latent_shape()                             # the preset's latent size
    meta = dict(meta, B=B, T=T, latent=[c, h, w])
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
    return meta, model, z_in, z_out, prm


def _prop(model):
    return {k: p for k, p in model.named_parameters() if k.startswith("propagator.")}


def _snapshot(model):
    return {k: p.detach().clone() for k, p in _prop(model).items()}


def _coef_of(tr):
    """The device coefficient of the trainer's last clipped step (include/lns.h: 768 bytes before the workspace's end)."""
    ws = [w for key, w in tr._ws.items() if key[-1]]
    assert len(ws) == 1
    return ws[0][-768:-764].view(torch.float32)[0]


def _unfused_steps(model, z_in, z_out, prm, K, max_norm, wgrad):
    """K steps of what a user writes today: step(update=False); torch.nn.utils.clip_grad_norm_; optim.Adam.step()."""
    from lns_amd import train
    tr = train.Stage2Trainer(model, lr=LR, wgrad=wgrad)
    params = list(_prop(model).values())
    traj, norms = [], []
    for _ in range(K):
        tr.step(z_in, z_out, prm, update=False)
        norms.append(torch.nn.utils.clip_grad_norm_(params, max_norm).clone())
        tr.optimizer.step()
        traj.append(_snapshot(model))
    return traj, norms


@pytest.mark.parametrize("wgrad", ["tile", "split"])
@pytest.mark.parametrize("case", STEP_CASES)
def test_clipped_step_matches_the_unfused_sequence(case, wgrad):
    """ns2d_mini (B = 4, T = 2) and twophase_cond at its preset latent size (B = 2, T = 2), both weight-gradient forms,
    max_grad_norm = half the norm of an update=False step on the same batch, so the clip is active at step 1.
    After one step: `.grad` = unclipped gradient x the device coefficient within 2 ulp; the coefficient within 1 ulp of
    clip_grad_norm_'s formula; trainer.grad_norm within 1e-6 of torch's norm, the float64 norm the arbiter.  After K = 5
    steps the fused trainer's distance from the unfused sequence, relative to how far that moved, is gated by the rule of
    tests/test_train_step_gpu.py::test_step_matches_the_autograd_path (its line 346): at most max(1e-4, 3 x the path's own
    fp32 spread), the spread being the unfused sequence re-run with its batch rows reversed."""
    _need_gpu()
    from lns_amd import train
    K = 5
    meta, model_f, z_in, z_out, prm = _setup(case)
    assert tuple(z_out.shape[:2]) == BATCH[case] and tuple(z_out.shape[2:]) == tuple(model_f._eng.latent_shape())
    init = _snapshot(model_f)
    probe = train.Stage2Trainer(model_f, lr=LR, wgrad=wgrad)
    probe.step(z_in, z_out, prm, update=False)
    g0 = {k: p.grad.detach().clone() for k, p in _prop(model_f).items()}
    norm64 = _norm64(list(g0.values()))
    # torch's own norm of the same gradients: clip_grad_norm_'s fp32 norm of the per-tensor fp32 norms
    torch_norm = float(torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g) for g in g0.values()])).item())
    max_norm = 0.5 * norm64
    tr = train.Stage2Trainer(model_f, lr=LR, wgrad=wgrad, max_grad_norm=max_norm)
    assert all(torch.equal(p.detach(), init[k]) for k, p in _prop(model_f).items())
    traj_f = []
    tr.step(z_in, z_out, prm)
    norm1, coef1 = float(tr.grad_norm.item()), _coef_of(tr).cpu().numpy()
    g1 = {k: p.grad.detach().clone() for k, p in _prop(model_f).items()}
    traj_f.append(_snapshot(model_f))
    for _ in range(K - 1):
        tr.step(z_in, z_out, prm)
        traj_f.append(_snapshot(model_f))
    # step 1
    c_ulp = _ulp_err(np.array([coef1]), np.array([_coef64(np.float32(norm1), max_norm)]))
    g_ulp = max(_ulp_err(g1[k].cpu().numpy(), g0[k].cpu().numpy().astype(np.float64) * float(coef1)) for k in g0)
    n_rel_torch, n_rel_64 = abs(norm1 - torch_norm) / norm64, abs(norm1 - norm64) / norm64
    assert 0.49 < float(coef1) < 0.51 and c_ulp <= 1.0, (coef1, c_ulp)
    assert g_ulp <= 2.0, g_ulp
    assert n_rel_64 <= 1e-6 and (n_rel_torch <= 1e-6 or n_rel_64 <= abs(torch_norm - norm64) / norm64), (norm1, torch_norm, norm64)
    # K steps against the unfused sequence and its own spread
    _, model_u, _, _, _ = _setup(case)
    traj_u, norms_u = _unfused_steps(model_u, z_in, z_out, prm, K, max_norm, wgrad)
    _, model_r, rz_in, rz_out, rprm = _setup(case, reverse=True)
    traj_r, _ = _unfused_steps(model_r, rz_in, rz_out, rprm, K, max_norm, wgrad)
    torch.cuda.synchronize()

    def spread(traj):
        out = {}
        for k in init:
            moved = [float((traj_u[i][k] - init[k]).norm()) for i in range(K)]
            out[k] = max(float((traj[i][k] - traj_u[i][k]).norm()) / moved[i] for i in range(K) if moved[i] > 0)
        return out
    own, ours = spread(traj_r), spread(traj_f)
    k_own, k_ours = max(own, key=own.get), max(ours, key=ours.get)
    record = dict(case=case, wgrad=wgrad, K=K, lr=LR, max_grad_norm=max_norm, grad_norm_float64=norm64, grad_norm_trainer=norm1,
                  grad_norm_torch=torch_norm, grad_norm_unfused_step1=float(norms_u[0].item()), coef=float(coef1), coef_ulp=c_ulp,
                  clipped_grad_ulp_max=g_ulp, own_spread_max=own[k_own], own_spread_tensor=k_own,
                  fused_vs_unfused_max=ours[k_ours], fused_vs_unfused_tensor=k_ours)
    print("train_clip_parity", json.dumps(record))
    if os.environ.get("LNS_WRITE_PROFILES"):                # the committed record is written on request only, as train_step_parity.json is
        path = os.path.join(ROOT, "profiles", "train_clip_parity.json")
        allr = json.load(open(path)) if os.path.exists(path) else {}
        allr["%s/%s" % (case, wgrad)] = record
        with open(path, "w") as f:
            json.dump(allr, f, indent=1, sort_keys=True)
    for k in init:
        assert ours[k] <= max(1e-4, 3.0 * own[k]), (k, ours[k], own[k])
    assert all(float(tr.optimizer.state[p]["step"]) == K for p in _prop(model_f).values())


def test_inactive_clip_is_bit_identical_to_the_plain_trainer():
    """max_grad_norm = 1e30: the coefficient is exactly 1 and three steps leave the bits a plain Stage2Trainer leaves -- the
    clipped kernel's arithmetic is adam_multi_kernel's."""
    _need_gpu()
    from lns_amd import train
    _, model_a, z_in, z_out, prm = _setup("ns2d_mini")
    _, model_b, _, _, _ = _setup("ns2d_mini")
    plain = train.Stage2Trainer(model_a, lr=LR, weight_decay=1e-2)
    clip = train.Stage2Trainer(model_b, lr=LR, weight_decay=1e-2, max_grad_norm=1e30)
    for _ in range(3):
        la = plain.step(z_in, z_out, prm).clone()
        lb = clip.step(z_in, z_out, prm).clone()
        assert float(_coef_of(clip).item()) == 1.0
        assert torch.equal(la.view(torch.int32), lb.view(torch.int32))
    pa, pb = _prop(model_a), _prop(model_b)
    for k in pa:
        assert torch.equal(pa[k].detach().view(torch.int32), pb[k].detach().view(torch.int32)), k
        assert torch.equal(pa[k].grad.view(torch.int32), pb[k].grad.view(torch.int32)), k
        for name in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(plain.optimizer.state[pa[k]][name].view(torch.int32), clip.optimizer.state[pb[k]][name].view(torch.int32)), (k, name)
    assert int(clip.skipped_steps.item()) == 0 and np.isfinite(clip.grad_norm.item())


def test_trainer_adamw_step_is_the_optimisers_own_step():
    """Stage2Trainer with an lns_amd.optim.AdamW: one fused step leaves the bits of step(update=False) + AdamW.step(), and
    not those of the L2 form."""
    _need_gpu()
    from lns_amd import optim, train
    _, model_a, z_in, z_out, prm = _setup("ns2d_mini")
    _, model_b, _, _, _ = _setup("ns2d_mini")
    _, model_c, _, _, _ = _setup("ns2d_mini")
    fused = train.Stage2Trainer(model_a, optimizer=optim.AdamW(model_a.propagator.parameters(), lr=LR, weight_decay=0.1))
    apart = train.Stage2Trainer(model_b, optimizer=optim.AdamW(model_b.propagator.parameters(), lr=LR, weight_decay=0.1))
    l2 = train.Stage2Trainer(model_c, lr=LR, weight_decay=0.1)
    for _ in range(2):
        fused.step(z_in, z_out, prm)
        apart.step(z_in, z_out, prm, update=False)
        apart.optimizer.step()
        l2.step(z_in, z_out, prm)
    pa, pb, pc = _prop(model_a), _prop(model_b), _prop(model_c)
    assert all(torch.equal(pa[k].detach().view(torch.int32), pb[k].detach().view(torch.int32)) for k in pa)
    assert any(not torch.equal(pa[k].detach(), pc[k].detach()) for k in pa)
    assert fused.grad_norm is not None and np.isfinite(fused.grad_norm.item())


def test_skip_nonfinite_leaves_everything_alone():
    """A non-finite gradient norm under skip_nonfinite: parameters, exp_avg, exp_avg_sq keep their bits, skipped_steps reads 1,
    grad_norm is non-finite, the next clean step updates; without the flag the same batch makes the parameters non-finite,
    which is what clip_grad_norm_ + Adam do.

    The batch that does this is one NaN in z_out.  One inf in z_out does NOT: smooth-L1's gradient outside |d| < beta is
    sign(d) / N, so pred - inf gives a finite gradient (and an infinite loss) -- in torch.nn.functional.smooth_l1_loss as
    in the kernel -- the norm stays finite and nothing is skipped, with or without the flag.  Both batches are checked."""
    _need_gpu()
    from lns_amd import train
    _, model, z_in, z_out, prm = _setup("ns2d_mini")
    nan_out, inf_out = z_out.clone(), z_out.clone()
    nan_out.view(-1)[nan_out.numel() // 2 + 5] = float("nan")
    inf_out.view(-1)[inf_out.numel() // 2 + 5] = float("inf")
    tr = train.Stage2Trainer(model, lr=LR, skip_nonfinite=True)
    tr.step(z_in, z_out, prm)                                         # a clean step first: the moments are not zero
    assert int(tr.skipped_steps.item()) == 0 and np.isfinite(tr.grad_norm.item())
    before = _snapshot(model)
    state = {k: {n: tr.optimizer.state[p][n].clone() for n in ("exp_avg", "exp_avg_sq")} for k, p in _prop(model).items()}
    loss = tr.step(z_in, nan_out, prm)
    assert not np.isfinite(tr.grad_norm.item()) and not np.isfinite(loss.item())
    assert int(tr.skipped_steps.item()) == 1
    for k, p in _prop(model).items():
        assert torch.equal(p.detach().view(torch.int32), before[k].view(torch.int32)), k
        for n in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(tr.optimizer.state[p][n].view(torch.int32), state[k][n].view(torch.int32)), (k, n)
    assert any(not torch.isfinite(p.grad).all() for p in _prop(model).values())        # the raw gradients are left to look at
    assert all(float(tr.optimizer.state[p]["step"]) == 2.0 for p in _prop(model).values())   # the host count moves on (documented)
    loss = tr.step(z_in, z_out, prm)
    assert np.isfinite(loss.item()) and np.isfinite(tr.grad_norm.item()) and int(tr.skipped_steps.item()) == 1
    assert all(torch.isfinite(p).all() for p in _prop(model).values())
    assert all(not torch.equal(p.detach(), before[k]) for k, p in _prop(model).items())
    # an inf target: infinite loss, finite gradient, an ordinary update
    before = _snapshot(model)
    loss = tr.step(z_in, inf_out, prm)
    assert np.isinf(loss.item()) and np.isfinite(tr.grad_norm.item()) and int(tr.skipped_steps.item()) == 1
    assert all(torch.isfinite(p).all() and not torch.equal(p.detach(), before[k]) for k, p in _prop(model).items())
    # without the flag the NaN goes through, as it does through clip_grad_norm_ and Adam
    _, model2, _, _, _ = _setup("ns2d_mini")
    tr2 = train.Stage2Trainer(model2, lr=LR, max_grad_norm=1.0)
    tr2.step(z_in, nan_out, prm)
    assert not np.isfinite(tr2.grad_norm.item()) and int(tr2.skipped_steps.item()) == 0
    assert any(not torch.isfinite(p).all() for p in _prop(model2).values())


def test_default_trainer_never_takes_the_clipped_path(monkeypatch):
    """Neither argument and an optim.Adam: the step calls what it called before -- never lns_train_step_clip -- and its
    workspace has the size lns_train_step_workspace_bytes returns."""
    _need_gpu()
    from lns_amd import engine, optim, train
    meta, model, z_in, z_out, prm = _setup("ns2d_mini")

    def boom(*a, **k):
        raise AssertionError("the plain trainer went through the clipped entry point")
    monkeypatch.setattr(engine.Engine, "train_step_clip", boom)
    monkeypatch.setattr(engine.Engine, "train_step_clip_workspace_bytes", boom)
    for opt in (None, optim.Adam(model.propagator.parameters(), lr=LR)):
        tr = train.Stage2Trainer(model, optimizer=opt, lr=LR)
        assert not tr.clipped
        tr.step(z_in, z_out, prm)
        tr.step(z_in, z_out, prm, update=False)
        c, h, w = meta["latent"]
        assert [ws.numel() for ws in tr._ws.values()] == [model._eng.train_step_workspace_bytes(meta["B"], h, w, meta["T"])]
        assert tr.grad_norm is None and int(tr.skipped_steps.item()) == 0
    assert np.isfinite(tr.step(z_in, z_out, prm).item())

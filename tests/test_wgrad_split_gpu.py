"""GPU: the batch-parallel weight gradient (option "train_wgrad" = 1; csrc/wgrad_split.inc).  Op level: both forms of
lns_op_conv_wgrad against a float64 numpy evaluation through index maps built as the oracle builds them
(oracle/lns_oracle.c lo_src_index).  Training: Stage2Trainer(wgrad="split") under the comparisons of
tests/test_train_step_gpu.py -- same fixtures, same tolerances, same rules."""
import itertools
import json
import os

import numpy as np
import pytest
import torch

import test_train_step_gpu as base
from helpers import ROOT, rel_l2

pytestmark = pytest.mark.gpu

PARITY = 2e-6                      # the project's per-kernel parity bound
ZEROS, CIRC = 0, 1
PADS = [(CIRC, CIRC), (ZEROS, ZEROS), (ZEROS, CIRC)]           # (pad_y, pad_x); the last one is the half-periodic propagator
SIZES = [(8, 8), (16, 16), (12, 24), (7, 15)]
BATCHES = [1, 3, 32]
GEOM_3x3 = [(128, 128, 3, 1), (128, 128, 3, 2), (128, 128, 3, 3), (40, 72, 3, 2)]      # (Cin, Cout, k, dilation)
GEOM_1x1 = [(16, 128, 1, 1), (128, 16, 1, 1), (128, 128, 1, 1), (72, 40, 1, 1)]


def _cases():
    """Every 3x3 geometry x padding x latent size and every 1x1 geometry x latent size, the batch sizes (and, for 1x1, the
    paddings, which a 1x1 never reads) cycling so that each B meets each size and each padding."""
    out = []
    for n, (g, pad, hw) in enumerate(itertools.product(GEOM_3x3, PADS, SIZES)):
        out.append(g + pad + hw + (BATCHES[(n + n // 4) % 3],))
    for n, (g, hw) in enumerate(itertools.product(GEOM_1x1, SIZES)):
        out.append(g + PADS[n % 3] + hw + (BATCHES[(n + n // 4) % 3],))
    # 3x3 whose x patch ((rows of a chunk + 2 dil) x (W + 2 dil) = 9 x 62 / 10 x 72 > 512 positions) does not fit: the
    # batch-parallel form takes its other kernel, the nine taps on the grid
    out += [(128, 128, 3, 3, ZEROS, CIRC, 8, 56, 3), (128, 128, 3, 3, CIRC, CIRC, 8, 56, 1), (40, 72, 3, 4, ZEROS, ZEROS, 5, 64, 32)]
    return out


def _axis_map(n, p, mode):
    """padded coordinate 0 .. n + 2p - 1 -> source index, or -1 (zero)"""
    out = []
    for q in range(n + 2 * p):
        u = q - p
        if 0 <= u < n:
            out.append(u)
        else:
            out.append(u % n if mode == CIRC else -1)
    return np.array(out)


def _ref64(dy, x, k, dil, pad_y, pad_x):
    B, Cout, H, W = dy.shape
    Cin = x.shape[1]
    p = dil * (k - 1) // 2
    rm, cm = _axis_map(H, p, pad_y), _axis_map(W, p, pad_x)
    x64 = x.astype(np.float64)
    d2 = dy.astype(np.float64).transpose(1, 0, 2, 3).reshape(Cout, -1)
    dw = np.empty((Cout, Cin, k, k), np.float64)
    for ty in range(k):
        for tx in range(k):
            r, c = rm[ty * dil: ty * dil + H], cm[tx * dil: tx * dil + W]
            xs = x64[:, :, np.maximum(r, 0)][:, :, :, np.maximum(c, 0)]
            xs = xs * ((r >= 0)[:, None] & (c >= 0)[None, :])
            dw[:, :, ty, tx] = d2 @ xs.transpose(1, 0, 2, 3).reshape(Cin, -1).T
    return dw


def _engine():
    from lns_amd import config, engine
    a = config.preset("ns2d_mini")
    return engine.Engine(engine.make_config(a, ae_prefix="vq_ae.", prop_prefix="propagator."))


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("Cin,Cout,k,dil,pad_y,pad_x,H,W,B", _cases())
def test_op_both_forms_match_float64(Cin, Cout, k, dil, pad_y, pad_x, H, W, B):
    """rel-L2 of form 1 <= max(2e-6, 2 x rel-L2 of form 0 on the same inputs), accumulate 0 and 1; form 1 twice gives equal
    bits; form 0 gives the same bits before and after form 1 ran on the engine."""
    base._need_gpu()
    e = _engine()
    rng = np.random.default_rng(1000 * Cin + 10 * Cout + 7 * k + dil + 3 * H + W + B + 5 * pad_y + pad_x)
    dy = rng.standard_normal((B, Cout, H, W)).astype(np.float32)
    x = rng.standard_normal((B, Cin, H, W)).astype(np.float32)
    dw0 = (rng.standard_normal((Cout, Cin, k, k)) * np.sqrt(B * H * W)).astype(np.float32)     # the size of the sum itself
    ref = _ref64(dy, x, k, dil, pad_y, pad_x)
    tdy, tx = torch.from_numpy(dy).cuda(), torch.from_numpy(x).cuda()
    kw = dict(ksize=k, dilation=dil, pad_y=pad_y, pad_x=pad_x)
    tile_before = e.conv_wgrad(tdy, tx, form=0, **kw)
    split_a = e.conv_wgrad(tdy, tx, form=1, **kw)
    split_b = e.conv_wgrad(tdy, tx, form=1, **kw)
    tile_after = e.conv_wgrad(tdy, tx, form=0, **kw)
    acc = {}
    for form in (0, 1):
        acc[form] = e.conv_wgrad(tdy, tx, form=form, accumulate=True, dw=torch.from_numpy(dw0).cuda(), **kw)
    torch.cuda.synchronize()
    e0, e1 = rel_l2(tile_before.cpu().numpy(), ref), rel_l2(split_a.cpu().numpy(), ref)
    ref_acc = ref + dw0.astype(np.float64)
    a0, a1 = rel_l2(acc[0].cpu().numpy(), ref_acc), rel_l2(acc[1].cpu().numpy(), ref_acc)
    print("conv_wgrad %d->%d k%d d%d pad(%d,%d) %dx%d B=%d: rel-L2 tile %.3e split %.3e | accumulate: tile %.3e split %.3e"
          % (Cin, Cout, k, dil, pad_y, pad_x, H, W, B, e0, e1, a0, a1))
    assert np.isfinite(e1) and e1 <= max(PARITY, 2.0 * e0), (e1, e0)
    assert np.isfinite(a1) and a1 <= max(PARITY, 2.0 * a0), (a1, a0)
    assert torch.equal(_bits(split_a), _bits(split_b))
    assert torch.equal(_bits(tile_before), _bits(tile_after))


# ---- training ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", base.GRAD_CASES)
def test_split_gradients_pass_the_reference_fixture(case):
    """Stage2Trainer(wgrad="split").step(update=False) under the comparison of
    tests/test_train_step_gpu.py::test_step_gradients_pass_the_reference_fixture: GRAD_TOL = 1e-4 and the `3 x own` rule
    against the fp32 and fp64 runs of the real reference, on all four gradient fixtures."""
    base._need_gpu()
    from lns_amd import train
    g, meta, model, z_in, z_out, prm = base._setup(case)
    before = {k: p.detach().clone() for k, p in base._prop(model).items()}
    tr = train.Stage2Trainer(model, lr=base.LR, wgrad="split")
    assert model._owner._eng.options["train_wgrad"] == 1
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
        print("split grads %s %s: vs fp32 %.3e vs fp64 %.3e norm %.3e (reference's own %.3e)" % (case, k, e32, e64, en, own))
        assert e64 <= max(base.GRAD_TOL, 3.0 * own), (k, e32, e64, own)
        assert e32 <= max(base.GRAD_TOL, 3.0 * own), (k, e32, e64, own)
        assert en <= max(base.GRAD_TOL, 3.0 * own), (k, en)
    for k, p in base._prop(model).items():
        assert torch.equal(p.detach(), before[k]), k


def _trainer_steps(case, wgrad, K, with_state=False):
    from lns_amd import train
    _, _, model, z_in, z_out, prm = base._setup(case)
    tr = train.Stage2Trainer(model, lr=base.LR, wgrad=wgrad)
    losses, traj = [], []
    for _ in range(K):
        losses.append(tr.step(z_in, z_out, prm).clone())
        traj.append({k: p.detach().clone() for k, p in base._prop(model).items()})
    torch.cuda.synchronize()
    if with_state:
        st = {k: (tr.optimizer.state[p]["exp_avg"].clone(), tr.optimizer.state[p]["exp_avg_sq"].clone()) for k, p in base._prop(model).items()}
        return [l.item() for l in losses], traj, st
    return [l.item() for l in losses], traj


@pytest.mark.parametrize("case", base.STEP_CASES)
def test_five_split_steps_stay_within_the_autograd_spread_of_five_tile_steps(case):
    """K = 5 trainer steps with option 1 against K with option 0 on the same batch: the distance, relative to how far the
    option-0 parameters moved, is at most max(1e-4, 3 x the batch-reversed spread of the autograd path) -- the rule of
    tests/test_train_step_gpu.py::test_step_matches_the_autograd_path."""
    base._need_gpu()
    K = 5
    _, _, model_a, z_in, z_out, prm = base._setup(case)
    init = {k: p.detach().clone() for k, p in base._prop(model_a).items()}
    _, _, traj_a = base._autograd_steps(model_a, z_in, z_out, prm, K)
    _, _, model_r, rz_in, rz_out, rprm = base._setup(case, reverse=True)
    _, _, traj_r = base._autograd_steps(model_r, rz_in, rz_out, rprm, K)
    loss_t, traj_t = _trainer_steps(case, "tile", K)
    loss_s, traj_s = _trainer_steps(case, "split", K)

    def spread(traj, ref):
        out = {}
        for k in init:
            moved = [float((ref[i][k] - init[k]).norm()) for i in range(K)]
            out[k] = max(float((traj[i][k] - ref[i][k]).norm()) / moved[i] for i in range(K) if moved[i] > 0)
        return out
    own, ours = spread(traj_r, traj_a), spread(traj_s, traj_t)
    k_own, k_ours = max(own, key=own.get), max(ours, key=ours.get)
    record = dict(case=case, K=K, lr=base.LR, own_spread_max=own[k_own], own_spread_tensor=k_own, split_vs_tile_max=ours[k_ours],
                  split_vs_tile_tensor=k_ours, step1_loss_rel=abs(loss_s[0] - loss_t[0]) / abs(loss_t[0]), loss_tile=loss_t,
                  loss_split=loss_s)
    print("train_step_parity_wgrad", json.dumps(record))
    if os.environ.get("LNS_WRITE_PROFILES"):                # the committed record is written on request only
        path = os.path.join(ROOT, "profiles", "train_step_parity_wgrad.json")
        allr = json.load(open(path)) if os.path.exists(path) else {}
        allr[case] = record
        with open(path, "w") as f:
            json.dump(allr, f, indent=1, sort_keys=True)
    assert loss_s[0] == loss_t[0]                            # the forward pass does not depend on the option
    for k in init:
        assert ours[k] <= max(1e-4, 3.0 * own[k]), (k, ours[k], own[k])
    assert loss_s[-1] < loss_s[0], loss_s


@pytest.mark.parametrize("case", base.STEP_CASES)
def test_split_steps_are_bit_reproducible(case):
    """Two runs of the same five steps from the same state with option 1: bit-equal parameters and Adam moments."""
    base._need_gpu()
    la, ta, sa = _trainer_steps(case, "split", 5, with_state=True)
    lb, tb, sb = _trainer_steps(case, "split", 5, with_state=True)
    assert la == lb
    for k in ta[-1]:
        assert torch.equal(_bits(ta[-1][k]), _bits(tb[-1][k])), k
        assert torch.equal(_bits(sa[k][0]), _bits(sb[k][0])) and torch.equal(_bits(sa[k][1]), _bits(sb[k][1])), k


def test_no_hidden_work_in_the_split_step():
    """The check of tests/test_train_step_gpu.py::test_no_hidden_work_in_the_step with option 1: after the warm-up steps, 20
    steps allocate nothing, torch sees no synchronisation, .grad keeps its storage, the autoencoder is untouched."""
    base._need_gpu()
    from lns_amd import train
    _, _, model, z_in, z_out, _ = base._setup("ns2d_mini")
    tr = train.Stage2Trainer(model, lr=base.LR, wgrad="split")
    ae_before = {k: p.detach().clone() for k, p in model._ae.named_parameters()}
    for _ in range(2):
        tr.step(z_in, z_out)
    torch.cuda.synchronize()
    prop = base._prop(model)
    ptrs = {k: p.grad.data_ptr() for k, p in prop.items()}
    n0 = torch.cuda.memory_stats()["allocation.all.allocated"]
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(20):
            loss = tr.step(z_in, z_out)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    n1 = torch.cuda.memory_stats()["allocation.all.allocated"]
    torch.cuda.synchronize()
    assert n1 == n0, (n0, n1)
    assert np.isfinite(loss.item())
    assert all(p.grad.data_ptr() == ptrs[k] for k, p in prop.items())
    for k, p in model._ae.named_parameters():
        assert p.grad is None and torch.equal(p.detach(), ae_before[k]), k


def test_switching_the_form_on_a_live_trainer():
    """tile -> split -> tile on one trainer.  The split phase computes gradients only (update=False), so the final tile phase
    starts from the state a never-switched trainer has: its steps give the same bits.  One workspace per form is allocated,
    once; none is handed to the C call under the other option (that call would be refused with LNS_ENOMEM)."""
    base._need_gpu()
    from lns_amd import train

    def run(switch):
        _, _, model, z_in, z_out, prm = base._setup("twophase_cond")
        tr = train.Stage2Trainer(model, lr=base.LR, wgrad="tile")
        for _ in range(2):
            tr.step(z_in, z_out, prm)
        tile_ws = next(iter(tr._ws.values())).data_ptr()
        if switch:
            tr.set_wgrad("split")
        mid = [tr.step(z_in, z_out, prm, update=False).clone() for _ in range(2)]
        mid_grads = {k: p.grad.detach().clone() for k, p in base._prop(model).items()}
        if switch:
            assert len(tr._ws) == 2
            sizes = sorted(w.numel() for w in tr._ws.values())
            assert sizes[0] < sizes[1]
            tr.set_wgrad("tile")
        losses = [tr.step(z_in, z_out, prm).clone() for _ in range(3)]
        torch.cuda.synchronize()
        assert len(tr._ws) == (2 if switch else 1)
        assert tile_ws in [w.data_ptr() for w in tr._ws.values()]
        return [l.item() for l in mid], mid_grads, [l.item() for l in losses], {k: p.detach().clone() for k, p in base._prop(model).items()}
    mid_a, g_a, loss_a, p_a = run(False)
    mid_b, g_b, loss_b, p_b = run(True)
    assert mid_a == mid_b                                    # same forward
    worst = max(rel_l2(g_b[k].cpu().numpy(), g_a[k].cpu().numpy()) for k in g_a)
    assert worst <= 1e-5, worst                              # the step-1 gradient bound of test_step_matches_the_autograd_path
    assert loss_a == loss_b
    for k in p_a:
        assert torch.equal(_bits(p_a[k]), _bits(p_b[k])), k

"""CPU: the device-resident training step (lns_loss_smooth_l1, lns_adam_step{,_tensors}, lns_train_step & co.,
include/lns.h) is declared and exported, refuses bad arguments before any device work, sizes its workspace without a
GPU, and `lns_amd.optim.Adam` keeps torch.optim.Adam's state_dict layout while refusing CPU tensors."""
import ctypes
import os
import re

import pytest
import torch

from helpers import ROOT

STEP_SYMBOLS = ("lns_loss_smooth_l1", "lns_adam_step", "lns_adam_step_tensors", "lns_train_step_workspace_bytes", "lns_train_step")


def test_train_step_symbols_are_declared_and_exported():
    from lns_amd import _lib
    _lib.build()
    src = open(os.path.join(ROOT, "include", "lns.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(lns_[a-z0-9_]+)\s*\(", src))
    L = ctypes.CDLL(_lib.LIB_PATH)
    for s in STEP_SYMBOLS:
        assert s in declared, "not declared in include/lns.h: " + s
        assert hasattr(L, s), "missing export: " + s
        assert s in _lib.SYMBOLS
    assert "lns_adam_spec" in src and re.search(r"#define\s+LNS_ABI_VERSION\s+2\b", src)
    assert _lib.LNS_ABI_VERSION == 2


def _engine(preset="ns2d_mini", **kw):
    from lns_amd import config, engine
    a = config.preset(preset)
    return engine.Engine(engine.make_config(a, ae_prefix="ae." if a.family == "twophase_cond" else "vq_ae.",
                                            prop_prefix="propagator.", **kw))


def _arrays(e, fake=0x1000):
    """Four pointer arrays in table order with a fake (never dereferenced) device pointer for every propagator tensor."""
    out = []
    for _ in range(4):
        a = (ctypes.c_void_p * len(e.params))()
        for i, (k, _, isb) in enumerate(e.params):
            if k.startswith("propagator.") and not isb:
                a[i] = fake
        out.append(a)
    return out


def test_train_step_refuses_bad_arguments_without_a_device():
    """Every LNS_EINVAL / LNS_ESTATE / LNS_ENOMEM case is decided before the first HIP call: no GPU here, fake pointers."""
    from lns_amd import _lib, engine
    L = _lib.lib()
    e = _engine()
    h = e._h
    c, lh, lw = e.latent_shape()
    P = ctypes.c_void_p(0x1000)
    prm, grd, m, v = _arrays(e)
    good = engine.adam_spec(5e-4, step=1)

    def err():
        return L.lns_last_error(h).decode()

    def step(eng=h, params=prm, z_in=P, z_out=P, B=3, T=2, beta=1.0, grads=grd, ea=m, es=v, spec=good, loss=P, ws=P, nbytes=1 << 40):
        sp = ctypes.byref(spec) if spec is not None else None
        return L.lns_train_step(eng, params, z_in, z_out, None, B, lh, lw, T, beta, grads, ea, es, sp, loss, ws, nbytes, None)

    assert step(eng=None) == _lib.LNS_EINVAL

    def spec_with(**kw):
        s = engine.adam_spec(5e-4, step=1)
        for k, val in kw.items():
            setattr(s, k, val)
        return s
    cases = [(dict(beta=0.0), "beta"), (dict(beta=-1.0), "beta"), (dict(T=0), "T"), (dict(B=0), "B"), (dict(B=-1), "B"),
             (dict(loss=None), "loss_out"), (dict(z_in=None), "z_in"), (dict(z_out=None), "z_out"), (dict(params=None), "params"),
             (dict(grads=None), "grads"), (dict(ea=None), "exp_avg"), (dict(es=None), "exp_avg"),
             (dict(spec=spec_with(size=8)), "size"), (dict(spec=spec_with(size=32)), "size"), (dict(spec=spec_with(beta1=1.0)), "beta1"), (dict(spec=spec_with(beta1=-0.1)), "beta1"),
             (dict(spec=spec_with(beta2=1.0)), "beta2"), (dict(spec=spec_with(eps=0.0)), "eps"), (dict(spec=spec_with(lr=-1e-3)), "lr"),
             (dict(spec=spec_with(step=0)), "step")]
    for kw, word in cases:
        assert step(**kw) == _lib.LNS_EINVAL, kw
        assert word in err(), (kw, err())
    # a propagator parameter whose four pointers are only partly given
    first = next(i for i, (k, _, isb) in enumerate(e.params) if k.startswith("propagator.") and not isb)
    for which, word in ((0, "parameter"), (1, "gradient"), (2, "exp_avg"), (3, "exp_avg_sq")):
        arrs = _arrays(e)
        arrs[which][first] = None
        assert step(params=arrs[0], grads=arrs[1], ea=arrs[2], es=arrs[3]) == _lib.LNS_EINVAL
        assert word in err() and e.params[first][0] in err(), err()
    # ... which is fine for the optimiser state when no update is asked for (adam_spec == NULL); then the workspace is next
    assert step(spec=None, ea=None, es=None, nbytes=16) == _lib.LNS_ENOMEM
    # workspace: smaller than lns_train_step_workspace_bytes
    need = e.train_step_workspace_bytes(3, lh, lw, 2)
    assert step(nbytes=need - 1) == _lib.LNS_ENOMEM and "workspace" in err()
    assert step(ws=None) == _lib.LNS_ENOMEM
    # an engine without a propagator
    ae_only = _engine(prop_kind=_lib.LNS_PROP_NONE)
    a4 = _arrays(ae_only)
    assert L.lns_train_step(ae_only._h, a4[0], P, P, None, 3, lh, lw, 2, 1.0, a4[1], a4[2], a4[3], ctypes.byref(good), P, P, 1 << 40, None) \
        == _lib.LNS_ESTATE
    assert "propagator" in L.lns_last_error(ae_only._h).decode()
    nb = ctypes.c_size_t(0)
    assert L.lns_train_step_workspace_bytes(ae_only._h, 3, lh, lw, 2, ctypes.byref(nb)) == _lib.LNS_ESTATE       # one code for one condition
    # a loss tensor beyond the kernel's stated limit is refused, not truncated
    assert L.lns_loss_smooth_l1(P, P, (_lib.LNS_SL1_CHUNK << 30) + 1, 1.0, P, P, P, 1 << 40, None) == _lib.LNS_EINVAL
    # the conditional propagator needs param
    ce = _engine("twophase_cond")
    c4 = _arrays(ce)
    _, ch, cw = ce.latent_shape()
    assert L.lns_train_step(ce._h, c4[0], P, P, None, 2, ch, cw, 2, 1.0, c4[1], c4[2], c4[3], ctypes.byref(good), P, P, 1 << 40, None) \
        == _lib.LNS_EINVAL
    assert "param" in L.lns_last_error(ce._h).decode()


def test_loss_and_adam_entry_points_refuse_bad_arguments_without_a_device():
    from lns_amd import _lib, engine
    L = _lib.lib()
    P = ctypes.c_void_p(0x1000)

    def cerr():
        return L.lns_create_error().decode()
    for kw, code, word in ((dict(beta=0.0), _lib.LNS_EINVAL, "beta"), (dict(beta=-0.5), _lib.LNS_EINVAL, "beta"),
                           (dict(n=0), _lib.LNS_EINVAL, "n"), (dict(loss=None), _lib.LNS_EINVAL, "loss_out"),
                           (dict(pred=None), _lib.LNS_EINVAL, "pred"), (dict(nscratch=2), _lib.LNS_ENOMEM, "scratch"),
                           (dict(scratch=None), _lib.LNS_ENOMEM, "scratch")):
        a = dict(pred=P, target=P, n=3 * _lib.LNS_SL1_CHUNK, beta=1.0, loss=P, grad=P, scratch=P, nscratch=3)
        a.update(kw)
        rc = L.lns_loss_smooth_l1(a["pred"], a["target"], a["n"], a["beta"], a["loss"], a["grad"], a["scratch"], a["nscratch"], None)
        assert rc == code and word in cerr(), (kw, rc, cerr())
    e = _engine()
    prm, grd, m, v = _arrays(e)
    bad = engine.adam_spec(1e-3, step=0)
    assert L.lns_adam_step(e._h, prm, grd, m, v, ctypes.byref(bad), None) == _lib.LNS_EINVAL and "step" in L.lns_last_error(e._h).decode()
    assert L.lns_adam_step(e._h, prm, grd, m, v, None, None) == _lib.LNS_EINVAL
    assert L.lns_adam_step(e._h, None, grd, m, v, ctypes.byref(engine.adam_spec(1e-3)), None) == _lib.LNS_EINVAL
    assert L.lns_adam_step(None, prm, grd, m, v, ctypes.byref(engine.adam_spec(1e-3)), None) == _lib.LNS_EINVAL
    one = (ctypes.c_void_p * 1)(0x1000)
    big = (ctypes.c_int64 * 1)(1 << 31)
    assert L.lns_adam_step_tensors(1, one, one, one, one, big, ctypes.byref(engine.adam_spec(1e-3)), None) == _lib.LNS_EINVAL
    assert "elements" in cerr()
    assert L.lns_adam_step_tensors(1, one, one, one, one, (ctypes.c_int64 * 1)(5), ctypes.byref(engine.adam_spec(1e-3, eps=0.0)), None) == _lib.LNS_EINVAL
    assert "eps" in cerr()


@pytest.mark.parametrize("preset,B,T", [("ns2d_mini", 4, 2), ("ns2d_64", 32, 2), ("twophase_cond", 32, 5), ("sw_half_periodic", 32, 5)])
def test_step_workspace_is_sized_without_a_device(preset, B, T):
    """lns_train_step_workspace_bytes = lns_train_workspace_bytes + z_pred + dL/dz_pred + loss partials."""
    from lns_amd import _lib
    L = _lib.lib()
    e = _engine(preset)
    c, h, w = e.latent_shape()
    a, b = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert L.lns_train_workspace_bytes(e._h, B, h, w, T, ctypes.byref(a)) == 0, L.lns_last_error(e._h)
    assert L.lns_train_step_workspace_bytes(e._h, B, h, w, T, ctypes.byref(b)) == 0, L.lns_last_error(e._h)
    n = B * T * c * h * w
    assert b.value >= a.value + 2 * n * 4 + 4 * -(-n // _lib.LNS_SL1_CHUNK)
    assert b.value <= a.value + 2 * n * 4 + 4 * -(-n // _lib.LNS_SL1_CHUNK) + 4 * 256      # nothing else hides in it
    assert L.lns_train_step_workspace_bytes(e._h, 0, h, w, T, ctypes.byref(b)) == _lib.LNS_EINVAL
    assert L.lns_train_step_workspace_bytes(e._h, B, h, w, 0, ctypes.byref(b)) == _lib.LNS_EINVAL


def test_adam_refuses_cpu_tensors_and_unsupported_variants():
    from lns_amd import optim
    from lns_amd._lib import LnsError
    p = torch.nn.Parameter(torch.ones(5))
    opt = optim.Adam([p], lr=1e-3)
    p.grad = torch.ones(5)
    with pytest.raises(LnsError, match="no CPU fallback"):
        opt.step()
    assert torch.equal(p.detach(), torch.ones(5))
    for kw in (dict(amsgrad=True), dict(maximize=True), dict(capturable=True), dict(differentiable=True), dict(decoupled_weight_decay=True)):
        with pytest.raises(LnsError):
            optim.Adam([p], **kw)


def test_trainer_refuses_cpu_models_and_foreign_optimizers():
    from lns_amd import config, dropin, train
    from lns_amd._lib import LnsError
    m = dropin.build_dynamics(config.preset("ns2d_mini"))
    with pytest.raises(LnsError, match="no CPU fallback"):
        train.Stage2Trainer(m).step(torch.zeros(2, 1, 8, 4, 4), torch.zeros(2, 2, 8, 4, 4))
    with pytest.raises(LnsError, match="lns_amd.optim.Adam"):
        train.Stage2Trainer(m, optimizer=torch.optim.Adam(m.propagator.parameters()))
    with pytest.raises(LnsError):
        train.Stage2Trainer(torch.nn.Linear(2, 2))


def test_adam_state_dict_has_torch_layout():
    """A torch.optim.Adam that took two CPU steps -> its state_dict rebuilt by hand -> lns_amd.optim.Adam -> read back: the
    same keys, dtypes and values; and that state_dict loads into a fresh torch.optim.Adam."""
    from lns_amd import optim
    torch.manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(3, 4)), torch.nn.Parameter(torch.randn(7))]
    ref = torch.optim.Adam(ps, lr=2e-3, betas=(0.8, 0.95), eps=1e-7, weight_decay=1e-2)
    for _ in range(2):
        for p in ps:
            p.grad = torch.randn_like(p)
        ref.step()
    sd = ref.state_dict()
    by_hand = dict(state={i: dict(step=torch.tensor(2.0), exp_avg=sd["state"][i]["exp_avg"].clone(),
                                  exp_avg_sq=sd["state"][i]["exp_avg_sq"].clone()) for i in (0, 1)},
                   param_groups=[dict(sd["param_groups"][0])])
    ours = optim.Adam([torch.nn.Parameter(p.detach().clone()) for p in ps], lr=1.0)
    ours.load_state_dict(by_hand)
    back = ours.state_dict()
    assert set(back) == {"state", "param_groups"} and set(back["state"]) == {0, 1}
    g_ref, g_back = sd["param_groups"][0], back["param_groups"][0]
    assert set(g_back) == set(g_ref), (sorted(g_back), sorted(g_ref))
    for k in ("lr", "betas", "eps", "weight_decay", "amsgrad", "maximize", "params"):
        assert g_back[k] == g_ref[k], k
    for i in (0, 1):
        assert set(back["state"][i]) == {"step", "exp_avg", "exp_avg_sq"} == set(sd["state"][i])
        for k in ("step", "exp_avg", "exp_avg_sq"):
            a, b = back["state"][i][k], sd["state"][i][k]
            assert isinstance(a, torch.Tensor) and a.dtype == b.dtype and a.device == b.device and a.shape == b.shape, (i, k)
            assert torch.equal(a, b), (i, k)
    # a fresh lns Adam has exactly torch's param-group keys, and refuses a loaded group it does not compute
    assert set(optim.Adam([torch.nn.Parameter(torch.zeros(2))]).state_dict()["param_groups"][0]) == set(g_ref)
    if "decoupled_weight_decay" in g_ref:
        from lns_amd._lib import LnsError
        adamw_like = dict(state={}, param_groups=[dict(g_ref, decoupled_weight_decay=True)])
        with pytest.raises(LnsError, match="decoupled_weight_decay"):
            optim.Adam([torch.nn.Parameter(p.detach().clone()) for p in ps]).load_state_dict(adamw_like)
    # a fresh (never stepped) lns Adam creates the same per-parameter layout as torch's lazily initialised state
    st = ours.init_state(torch.nn.Parameter(torch.zeros(2)))
    assert set(st) == {"step", "exp_avg", "exp_avg_sq"} and st["step"].dtype == torch.float32 and st["step"].device.type == "cpu"
    # and back into torch
    again = torch.optim.Adam([torch.nn.Parameter(p.detach().clone()) for p in ps])
    again.load_state_dict(back)
    for p in again.param_groups[0]["params"]:
        p.grad = torch.ones_like(p)
    again.step()
    assert float(again.state[again.param_groups[0]["params"][0]]["step"]) == 3.0
    # CosineAnnealingLR drives it like any torch optimiser
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(ours, T_max=10)
    lr0 = ours.param_groups[0]["lr"]
    ours.zero_grad()
    sched.step()
    assert ours.param_groups[0]["lr"] < lr0

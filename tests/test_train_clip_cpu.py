"""CPU: gradient-norm clipping and AdamW of the training step (include/lns.h "gradient-norm clipping and AdamW"):
lns_grad_norm_*, lns_update_step_tensors and lns_train_step_clip are declared and exported, refuse bad arguments before
any device work (fake pointers, no GPU here), size their scratch and workspace on the host, and `lns_amd.optim.AdamW`
keeps torch.optim.AdamW's state_dict layout."""
import ctypes
import math
import os
import re

import pytest
import torch

from helpers import ROOT

CLIP_SYMBOLS = ("lns_grad_norm_scratch_bytes", "lns_grad_norm_tensors", "lns_grad_scale_tensors", "lns_update_step_tensors",
                "lns_train_step_clip_workspace_bytes", "lns_train_step_clip")


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


def _round256(n):
    return -(-n // 256) * 256


def test_clip_symbols_are_declared_exported_and_announced():
    from lns_amd import _lib
    _lib.build()
    src = open(os.path.join(ROOT, "include", "lns.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(lns_[a-z0-9_]+)\s*\(", code))
    L = _lib.lib()
    for s in CLIP_SYMBOLS:
        assert s in declared and hasattr(L, s) and s in _lib.SYMBOLS, s
    assert re.search(r"#define\s+LNS_ABI_VERSION\s+2\b", src)                      # additive: the version stays
    assert L.lns_build_has(b"train_clip") == 1
    assert ctypes.sizeof(_lib.LnsUpdateSpec) == 64 and ctypes.sizeof(_lib.LnsAdamSpec) == 56
    assert re.search(r"#define\s+LNS_NORM_CHUNK\s+%d\b" % _lib.LNS_NORM_CHUNK, src)
    assert re.search(r"#define\s+LNS_UPDATE_DECOUPLED_WD\s+1u?\b", src) and re.search(r"#define\s+LNS_UPDATE_SKIP_NONFINITE\s+2u?\b", src)


def test_train_step_clip_refuses_bad_arguments_without_a_device():
    from lns_amd import _lib, engine
    L = _lib.lib()
    e = _engine()
    h = e._h
    c, lh, lw = e.latent_shape()
    P = ctypes.c_void_p(0x1000)
    prm, grd, m, v = _arrays(e)
    good = engine.update_spec(5e-4, step=1, max_norm=1.0)

    def err():
        return L.lns_last_error(h).decode()

    def step(eng=h, params=prm, z_in=P, z_out=P, B=3, T=2, beta=1.0, grads=grd, ea=m, es=v, spec=good, loss=P, norm=P, ws=P, nbytes=1 << 40):
        sp = ctypes.byref(spec) if spec is not None else None
        return L.lns_train_step_clip(eng, params, z_in, z_out, None, B, lh, lw, T, beta, grads, ea, es, sp, loss, norm, ws, nbytes, None)

    def spec_with(**kw):
        s = engine.update_spec(5e-4, step=1, max_norm=1.0)
        for k, val in kw.items():
            setattr(s, k, val)
        return s
    assert step(eng=None) == _lib.LNS_EINVAL
    cases = [(dict(spec=spec_with(size=56)), "size"), (dict(spec=spec_with(size=72)), "size"), (dict(spec=None), "spec"),
             (dict(spec=spec_with(flags=4)), "flags"), (dict(spec=spec_with(flags=0x80000001)), "flags"),
             (dict(spec=spec_with(max_norm=float("nan"))), "max_norm"), (dict(spec=spec_with(step=0)), "step"),
             (dict(spec=spec_with(step=-3)), "step"), (dict(spec=spec_with(lr=-1e-3)), "lr"), (dict(spec=spec_with(eps=0.0)), "eps"),
             (dict(spec=spec_with(beta1=1.0)), "beta1"), (dict(spec=spec_with(beta2=-0.5)), "beta2"),
             (dict(spec=spec_with(weight_decay=-1.0)), "weight_decay"),
             (dict(params=None), "params"), (dict(grads=None), "grads"), (dict(ea=None), "exp_avg"), (dict(es=None), "exp_avg"),
             (dict(z_in=None), "z_in"), (dict(z_out=None), "z_out"), (dict(loss=None), "loss_out"), (dict(beta=0.0), "beta"),
             (dict(B=0), "B"), (dict(T=0), "T")]
    for kw, word in cases:
        assert step(**kw) == _lib.LNS_EINVAL, kw
        assert word in err(), (kw, err())
    # every valid flag combination and "no clipping" pass the spec check: the (short) workspace is what stops them
    for ok in (spec_with(flags=0), spec_with(flags=1), spec_with(flags=2), spec_with(flags=3), spec_with(max_norm=0.0),
               spec_with(max_norm=-1.0), spec_with(max_norm=float("inf"))):
        assert step(spec=ok, nbytes=16) == _lib.LNS_ENOMEM, err()
    # a propagator tensor with one of its four pointers missing
    first = next(i for i, (k, _, isb) in enumerate(e.params) if k.startswith("propagator.") and not isb)
    for which, word in ((0, "parameter"), (1, "gradient"), (2, "exp_avg"), (3, "exp_avg_sq")):
        arrs = _arrays(e)
        arrs[which][first] = None
        assert step(params=arrs[0], grads=arrs[1], ea=arrs[2], es=arrs[3]) == _lib.LNS_EINVAL
        assert word in err() and e.params[first][0] in err(), err()
    # workspace: the plain step's size is one tail short
    need = e.train_step_clip_workspace_bytes(3, lh, lw, 2)
    assert step(nbytes=need - 1) == _lib.LNS_ENOMEM and "workspace" in err() and str(need) in err()
    assert step(nbytes=e.train_step_workspace_bytes(3, lh, lw, 2)) == _lib.LNS_ENOMEM
    assert step(ws=None) == _lib.LNS_ENOMEM
    # an engine without a propagator: LNS_ESTATE from the step and from its size function
    ae_only = _engine(prop_kind=_lib.LNS_PROP_NONE)
    a4 = _arrays(ae_only)
    assert L.lns_train_step_clip(ae_only._h, a4[0], P, P, None, 3, lh, lw, 2, 1.0, a4[1], a4[2], a4[3], ctypes.byref(good), P, P, P,
                                 1 << 40, None) == _lib.LNS_ESTATE
    assert "propagator" in L.lns_last_error(ae_only._h).decode()
    nb = ctypes.c_size_t(0)
    assert L.lns_train_step_clip_workspace_bytes(ae_only._h, 3, lh, lw, 2, ctypes.byref(nb)) == _lib.LNS_ESTATE
    assert L.lns_train_step_clip_workspace_bytes(h, 0, lh, lw, 2, ctypes.byref(nb)) == _lib.LNS_EINVAL
    assert L.lns_train_step_clip_workspace_bytes(h, 3, lh, lw, 2, None) == _lib.LNS_EINVAL
    # the conditional propagator needs param
    ce = _engine("twophase_cond")
    c4 = _arrays(ce)
    _, ch, cw = ce.latent_shape()
    assert L.lns_train_step_clip(ce._h, c4[0], P, P, None, 2, ch, cw, 2, 1.0, c4[1], c4[2], c4[3], ctypes.byref(good), P, P, P,
                                 1 << 40, None) == _lib.LNS_EINVAL
    assert "param" in L.lns_last_error(ce._h).decode()


def test_norm_and_update_entry_points_refuse_bad_arguments_without_a_device():
    from lns_amd import _lib, engine
    L = _lib.lib()

    def cerr():
        return L.lns_create_error().decode()
    one = (ctypes.c_void_p * 1)(0x1000)
    five = (ctypes.c_int64 * 1)(5)
    big = (ctypes.c_int64 * 1)(1 << 31)
    zero = (ctypes.c_int64 * 1)(0)
    P = ctypes.c_void_p(0x1000)
    nb = ctypes.c_size_t(0)
    # scratch size
    assert L.lns_grad_norm_scratch_bytes(1, five, None) == _lib.LNS_EINVAL and "bytes" in cerr()
    assert L.lns_grad_norm_scratch_bytes(1, None, ctypes.byref(nb)) == _lib.LNS_EINVAL and "numel" in cerr()
    assert L.lns_grad_norm_scratch_bytes(-1, five, ctypes.byref(nb)) == _lib.LNS_EINVAL
    assert L.lns_grad_norm_scratch_bytes(1, big, ctypes.byref(nb)) == _lib.LNS_EINVAL and "elements" in cerr()
    assert L.lns_grad_norm_scratch_bytes(1, zero, ctypes.byref(nb)) == _lib.LNS_EINVAL and "elements" in cerr()
    # the norm
    def norm(n=1, grads=one, numel=five, max_norm=1.0, flags=0, scratch=P, nbytes=256):
        return L.lns_grad_norm_tensors(n, grads, numel, max_norm, P, P, None, flags, scratch, nbytes, None)
    for kw, code, word in ((dict(grads=None), _lib.LNS_EINVAL, "grads"), (dict(numel=None), _lib.LNS_EINVAL, "numel"),
                           (dict(numel=big), _lib.LNS_EINVAL, "elements"), (dict(max_norm=float("nan")), _lib.LNS_EINVAL, "max_norm"),
                           (dict(flags=4), _lib.LNS_EINVAL, "flags"), (dict(flags=0x10002), _lib.LNS_EINVAL, "flags"),
                           (dict(nbytes=255), _lib.LNS_ENOMEM, "scratch"), (dict(scratch=None), _lib.LNS_ENOMEM, "scratch")):
        assert norm(**kw) == code and word in cerr(), (kw, cerr())
    # the scale pass
    assert L.lns_grad_scale_tensors(1, None, five, P, None) == _lib.LNS_EINVAL and "grads" in cerr()
    assert L.lns_grad_scale_tensors(1, one, five, None, None) == _lib.LNS_EINVAL and "coef" in cerr()
    assert L.lns_grad_scale_tensors(1, one, big, P, None) == _lib.LNS_EINVAL and "elements" in cerr()
    # the update
    def upd(params=one, grads=one, ea=one, es=one, numel=five, spec=engine.update_spec(1e-3)):
        return L.lns_update_step_tensors(1, params, grads, ea, es, numel, ctypes.byref(spec) if spec is not None else None, None, None)

    def spec_with(**kw):
        s = engine.update_spec(1e-3)
        for k, val in kw.items():
            setattr(s, k, val)
        return s
    for kw, word in ((dict(params=None), "null"), (dict(grads=None), "null"), (dict(ea=None), "null"), (dict(es=None), "null"),
                     (dict(numel=None), "null"), (dict(numel=big), "elements"), (dict(spec=None), "spec"),
                     (dict(spec=spec_with(size=56)), "size"), (dict(spec=spec_with(flags=8)), "flags"),
                     (dict(spec=spec_with(max_norm=float("nan"))), "max_norm"), (dict(spec=spec_with(step=0)), "step"),
                     (dict(spec=spec_with(eps=0.0)), "eps")):
        assert upd(**kw) == _lib.LNS_EINVAL and word in cerr(), (kw, cerr())


def test_grad_norm_scratch_is_eight_bytes_per_chunk():
    """lns_grad_norm_scratch_bytes = 8 * sum(ceil(numel / LNS_NORM_CHUNK)), rounded up to 256 bytes (include/lns.h)."""
    from lns_amd import _lib
    L = _lib.lib()
    for sizes in ((1,), (2048,), (2049,), (1, 3, 2047, 2048, 2049, 5000), tuple(range(1, 98)), (2048 * 31 + 1,), (2048 * 32,),
                  ((1 << 31) - 1,), ()):
        nb = ctypes.c_size_t(123)
        arr = (ctypes.c_int64 * max(1, len(sizes)))(*sizes)
        assert L.lns_grad_norm_scratch_bytes(len(sizes), arr, ctypes.byref(nb)) == 0, L.lns_create_error()
        chunks = sum(-(-n // _lib.LNS_NORM_CHUNK) for n in sizes)
        assert nb.value == _round256(8 * chunks), (sizes, nb.value)
        assert nb.value - 8 * chunks < 256


@pytest.mark.parametrize("preset,B,T", [("ns2d_mini", 4, 2), ("twophase_cond", 32, 5), ("sw_half_periodic", 32, 5)])
def test_clip_workspace_is_the_step_workspace_plus_the_documented_tail(preset, B, T):
    """lns_train_step_clip_workspace_bytes - lns_train_step_workspace_bytes = norm partials (8 bytes per 2048-element chunk
    of every propagator tensor) + coefficient + norm + counter, each rounded up to 256 bytes -- exactly, under both
    weight-gradient forms; and lns_train_step_workspace_bytes itself is what it was."""
    from lns_amd import _lib
    e = _engine(preset)
    c, h, w = e.latent_shape()
    chunks = sum(-(-math.prod(shape) // _lib.LNS_NORM_CHUNK) for k, shape, isb in e.params if k.startswith("propagator.") and not isb)
    assert chunks > 0
    for form in (0, 1):
        e.set_option("train_wgrad", form)
        plain = e.train_step_workspace_bytes(B, h, w, T)
        clip = e.train_step_clip_workspace_bytes(B, h, w, T)
        assert plain % 256 == 0
        assert clip - plain == _round256(8 * chunks) + 3 * 256, (preset, form, clip - plain, chunks)


def test_adamw_state_dict_has_torch_layout():
    """A torch.optim.AdamW that took two CPU steps -> lns_amd.optim.AdamW -> read back: the same keys, dtypes and values;
    that state_dict loads into a fresh torch.optim.AdamW; Adam and AdamW refuse each other's param groups.  (The pattern of
    tests/test_train_step_cpu.py::test_adam_state_dict_has_torch_layout.)"""
    from lns_amd import optim
    from lns_amd._lib import LnsError
    torch.manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(3, 4)), torch.nn.Parameter(torch.randn(7))]
    ref = torch.optim.AdamW(ps, lr=2e-3, betas=(0.8, 0.95), eps=1e-7, weight_decay=3e-2)
    for _ in range(2):
        for p in ps:
            p.grad = torch.randn_like(p)
        ref.step()
    sd = ref.state_dict()

    def fresh():
        return [torch.nn.Parameter(p.detach().clone()) for p in ps]
    ours = optim.AdamW(fresh(), lr=1.0)
    assert isinstance(ours, torch.optim.Optimizer) and ours.defaults["weight_decay"] == 1e-2         # torch.optim.AdamW's default
    ours.load_state_dict(sd)
    back = ours.state_dict()
    assert set(back) == {"state", "param_groups"} and set(back["state"]) == {0, 1}
    g_ref, g_back = sd["param_groups"][0], back["param_groups"][0]
    assert set(g_back) == set(g_ref), (sorted(g_back), sorted(g_ref))
    for k in g_ref:
        assert g_back[k] == g_ref[k], k
    assert g_back["weight_decay"] == 3e-2 and g_back.get("decoupled_weight_decay", True) is True
    for i in (0, 1):
        assert set(back["state"][i]) == {"step", "exp_avg", "exp_avg_sq"} == set(sd["state"][i])
        for k in ("step", "exp_avg", "exp_avg_sq"):
            a, b = back["state"][i][k], sd["state"][i][k]
            assert isinstance(a, torch.Tensor) and a.dtype == b.dtype and a.device == b.device and a.shape == b.shape, (i, k)
            assert torch.equal(a, b), (i, k)
        assert float(back["state"][i]["step"]) == 2.0
    assert set(optim.AdamW([torch.nn.Parameter(torch.zeros(2))]).state_dict()["param_groups"][0]) == set(g_ref)
    # and back into torch
    again = torch.optim.AdamW(fresh())
    again.load_state_dict(back)
    for p in again.param_groups[0]["params"]:
        p.grad = torch.ones_like(p)
    again.step()
    assert float(again.state[again.param_groups[0]["params"][0]]["step"]) == 3.0
    # the two optimisers do not take each other's groups: which decay a checkpoint means is never guessed
    if "decoupled_weight_decay" in g_ref:
        with pytest.raises(LnsError, match="decoupled_weight_decay"):
            optim.Adam(fresh()).load_state_dict(sd)
        adam_sd = torch.optim.Adam(fresh(), weight_decay=1e-2).state_dict()
        with pytest.raises(LnsError, match="decoupled_weight_decay"):
            optim.AdamW(fresh()).load_state_dict(adam_sd)
    # no CPU path, and the variants the kernel does not compute raise
    p = torch.nn.Parameter(torch.ones(5))
    opt = optim.AdamW([p])
    p.grad = torch.ones(5)
    with pytest.raises(LnsError, match="no CPU fallback"):
        opt.step()
    assert torch.equal(p.detach(), torch.ones(5))
    for kw in (dict(amsgrad=True), dict(maximize=True), dict(capturable=True), dict(differentiable=True)):
        with pytest.raises(LnsError):
            optim.AdamW([p], **kw)


def test_adam_still_refuses_decoupled_weight_decay():
    from lns_amd import optim
    from lns_amd._lib import LnsError
    p = torch.nn.Parameter(torch.ones(5))
    with pytest.raises(LnsError):
        optim.Adam([p], decoupled_weight_decay=True)
    assert optim.Adam([p]).param_groups[0]["decoupled_weight_decay"] is False
    assert not isinstance(optim.Adam([p]), optim.AdamW) and isinstance(optim.AdamW([p]), optim.Adam)


def test_clip_grad_norm_refuses_what_it_does_not_compute():
    from lns_amd import optim
    from lns_amd._lib import LnsError
    p = torch.nn.Parameter(torch.ones(5))
    p.grad = torch.ones(5)
    for kw in (dict(norm_type=1.0), dict(norm_type=float("inf")), dict(error_if_nonfinite=True)):
        with pytest.raises(LnsError):
            optim.clip_grad_norm_([p], 1.0, **kw)
    with pytest.raises(LnsError, match="no CPU fallback"):
        optim.clip_grad_norm_([p], 1.0)
    assert torch.equal(p.grad, torch.ones(5))


def test_trainer_accepts_adamw_and_validates_the_new_arguments():
    from lns_amd import config, dropin, optim, train
    from lns_amd._lib import LnsError
    m = dropin.build_dynamics(config.preset("ns2d_mini"))
    plain = train.Stage2Trainer(m)
    assert not plain.clipped and plain.grad_norm is None
    assert train.Stage2Trainer(m, max_grad_norm=1.0).clipped and train.Stage2Trainer(m, skip_nonfinite=True).clipped
    assert train.Stage2Trainer(m, optimizer=optim.AdamW(m.propagator.parameters())).clipped
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(LnsError, match="max_grad_norm"):
            train.Stage2Trainer(m, max_grad_norm=bad)
    with pytest.raises(LnsError, match="lns_amd.optim.Adam"):
        train.Stage2Trainer(m, optimizer=torch.optim.AdamW(m.propagator.parameters()), max_grad_norm=1.0)


def test_new_kernels_use_no_scratch_and_spill_nothing():
    """tools/kernel_resources.py on the code object: the norm, finish, scale and update kernels have 0 scratch bytes and 0
    spilled registers (memory-bound elementwise kernels: anything else would be a regression)."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    from lns_amd import _lib
    res = kernel_resources.resources(_lib.LIB_PATH)
    for name in ("grad_sumsq_multi_kernel", "grad_norm_finish_kernel", "grad_scale_multi_kernel", "update_multi_kernel"):
        k = [v for n, v in res.items() if name in n]
        assert len(k) == 1, name
        assert k[0]["scratch"] == 0 and k[0]["vgpr_spill"] == 0 and k[0]["sgpr_spill"] == 0 and k[0]["vgpr"] <= 64, (name, k[0])

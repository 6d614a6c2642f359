"""CPU: the latent fit (include/lns.h "latent fit").  lns_train_backward_ex, lns_loss_obs_mse and lns_fit_step are
declared, exported and announced and refuse bad arguments before any device work (fake pointers, no GPU here); the float64
statement of the fit (tests/latent_fit_reference.py) does fit on the twin experiments; the inputs of the grad_param cases
tell deliberate mistakes of a hand-written backward from the truth; the gradients are well conditioned in float32."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import latent_fit_reference as lf
import train_reference as tr
from helpers import ROOT

FIT_SYMBOLS = ("lns_train_backward_ex", "lns_loss_obs_mse_scratch_bytes", "lns_loss_obs_mse", "lns_fit_step_workspace_bytes",
               "lns_fit_step")
P = ctypes.c_void_p(0x1000)


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


def test_fit_symbols_are_declared_exported_and_announced():
    from lns_amd import _lib
    _lib.build()
    src = open(os.path.join(ROOT, "include", "lns.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(lns_[a-z0-9_]+)\s*\(", code))
    L = _lib.lib()
    for s in FIT_SYMBOLS:
        assert s in declared and hasattr(L, s) and s in _lib.SYMBOLS, s
    assert re.search(r"#define\s+LNS_ABI_VERSION\s+2\b", src)                      # additive: the version stays
    assert L.lns_build_has(b"latent_fit") == 1
    assert ctypes.sizeof(_lib.LnsFitSpec) == 168 and ctypes.sizeof(_lib.LnsUpdateSpec) == 64
    assert re.search(r"#define\s+LNS_OBS_MAX\s+%d\b" % _lib.LNS_OBS_MAX, src)
    assert re.search(r"#define\s+LNS_FIT_STATE\s+1u?\b", src) and re.search(r"#define\s+LNS_FIT_PARAM\s+2u?\b", src)
    assert "no gradient w.r.t. it" not in src


def test_obs_loss_refuses_bad_arguments_without_a_device():
    from lns_amd import _lib
    L = _lib.lib()

    def cerr():
        return L.lns_create_error().decode()

    def call(z_pred=P, obs=P, B=2, T=5, n=63, steps=(1, 3), weights=(1.0, 0.5), z0=None, zb=None, lam=0.0, per=P, loss=P, grad=P,
             gbg=None, scratch=P, nbytes=1 << 20):
        st = (ctypes.c_int * max(1, len(steps)))(*steps) if steps is not None else None
        w = (ctypes.c_double * max(1, len(weights)))(*weights) if weights is not None else None
        return L.lns_loss_obs_mse(z_pred, obs, B, T, n, len(steps) if steps is not None else 1, st, w, z0, zb, lam, per, loss, grad, gbg,
                                  scratch, nbytes, None)
    cases = [(dict(z_pred=None), "z_pred"), (dict(obs=None), "obs"), (dict(loss=None), "loss"), (dict(grad=None), "grad_z_pred"),
             (dict(B=0), "B"), (dict(T=0), "T"), (dict(n=0), "n"), (dict(steps=None), "obs_steps"),
             (dict(steps=(3, 1)), "ascending"), (dict(steps=(1, 1)), "ascending"), (dict(steps=(-1, 2)), "ascending"),
             (dict(steps=(1, 5)), "below T"), (dict(weights=(1.0, -0.5)), "obs_weight"), (dict(weights=(float("nan"), 1.0)), "obs_weight"),
             (dict(weights=(float("inf"), 1.0)), "obs_weight"), (dict(steps=(), weights=()), "n_obs"),
             (dict(steps=tuple(range(65)), weights=(1.0,) * 65, T=70), "n_obs"), (dict(lam=-1.0, z0=P, zb=P), "background"),
             (dict(lam=float("nan"), z0=P, zb=P), "background"), (dict(lam=0.5), "z_background"), (dict(z0=P), "z_background"),
             (dict(zb=P), "z0"), (dict(gbg=P), "grad_z0_bg")]
    for kw, word in cases:
        assert call(**kw) == _lib.LNS_EINVAL, kw
        assert word in cerr(), (kw, cerr())
    need = _round256(8 * 2 * 3)
    assert call(nbytes=need - 1) == _lib.LNS_ENOMEM and str(need) in cerr()
    assert call(scratch=None) == _lib.LNS_ENOMEM
    nb = ctypes.c_size_t(0)
    for B, n_obs in ((1, 1), (3, 64), (33, 5)):
        assert L.lns_loss_obs_mse_scratch_bytes(B, n_obs, ctypes.byref(nb)) == 0 and nb.value == _round256(8 * B * (n_obs + 1))
    assert L.lns_loss_obs_mse_scratch_bytes(1, 0, ctypes.byref(nb)) == _lib.LNS_EINVAL
    assert L.lns_loss_obs_mse_scratch_bytes(1, 65, ctypes.byref(nb)) == _lib.LNS_EINVAL
    assert L.lns_loss_obs_mse_scratch_bytes(1, 1, None) == _lib.LNS_EINVAL


def test_backward_ex_and_fit_step_refuse_bad_arguments_without_a_device():
    from lns_amd import _lib, engine
    L = _lib.lib()
    e = _engine()
    h = e._h
    c, lh, lw = e.latent_shape()
    prm = _params(e)

    def err(eng=h):
        return L.lns_last_error(eng).decode()
    # lns_train_backward_ex: null pointers, and grad_param on a plain propagator -- all before any device work
    def bwd(params=prm, z_in=P, z_pred=P, g=P, B=2, T=2, grads=None, gz=P, gp=None):
        return L.lns_train_backward_ex(h, params, z_in, z_pred, g, B, lh, lw, T, grads, gz, P, 1 << 40, None, gp)
    for kw in (dict(params=None), dict(z_in=None), dict(z_pred=None), dict(g=None), dict(B=0), dict(T=0)):
        assert bwd(**kw) == _lib.LNS_EINVAL, kw
    assert bwd(gp=P) == _lib.LNS_EINVAL and "grad_param" in err()
    assert L.lns_train_backward(h, prm, P, P, P, 2, lh, lw, 2, None, P, P, 1 << 40, None) == _lib.LNS_EINVAL     # grads stay required there

    def spec_of(steps=(0, 2), weights=(1.0, 0.5), lam=0.0, state=True, param=False, **kw):
        s = engine.fit_spec(steps, weights, lam, state=(engine.update_spec(2e-3) if state is True else state) if state else None,
                            param=(engine.update_spec(1e-2) if param is True else param) if param else None)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def raw_spec(steps, weights):
        """a spec whose table fit_spec itself would refuse"""
        s = spec_of()
        s._steps = (ctypes.c_int * max(1, len(steps)))(*steps)
        s._weights = (ctypes.c_double * max(1, len(weights)))(*weights)
        s.obs_steps = ctypes.cast(s._steps, ctypes.POINTER(ctypes.c_int))
        s.obs_weight = ctypes.cast(s._weights, ctypes.POINTER(ctypes.c_double))
        s.n_obs = len(steps)
        return s

    def upd(**kw):
        u = engine.update_spec(2e-3)
        for k, v in kw.items():
            setattr(u, k, v)
        return u

    def step(eng=h, params=prm, z0=P, param=None, obs=P, zb=None, B=3, spec=None, gz=P, mz=P, vz=P, gp=None, mp=None, vp=None, loss=P,
             ws=P, nbytes=1 << 40, hh=lh, ww=lw):
        spec = spec_of() if spec is None else spec
        return L.lns_fit_step(eng, params, z0, param, obs, zb, B, hh, ww, ctypes.byref(spec) if spec != "null" else None, gz, mz, vz,
                              gp, mp, vp, loss, None, ws, nbytes, None)
    assert step(eng=None) == _lib.LNS_EINVAL
    cases = [(dict(spec="null"), "spec"), (dict(spec=spec_of(size=160)), "size"), (dict(spec=spec_of(flags=0)), "flags"),
             (dict(spec=spec_of(flags=4)), "flags"), (dict(spec=spec_of(flags=2)), "LNS_FIT_PARAM"),
             (dict(spec=spec_of(flags=3)), "LNS_FIT_PARAM"), (dict(params=None), "params"), (dict(z0=None), "z0"),
             (dict(obs=None), "obs"), (dict(loss=None), "loss"), (dict(gz=None), "g_z"), (dict(mz=None), "exp_avg_z"),
             (dict(vz=None), "exp_avg_sq_z"), (dict(B=0), "B"),
             (dict(spec=raw_spec((2, 0), (1.0, 1.0))), "ascending"), (dict(spec=raw_spec((0, 0), (1.0, 1.0))), "ascending"),
             (dict(spec=raw_spec((-1, 0), (1.0, 1.0))), "ascending"), (dict(spec=raw_spec((0, 1 << 24), (1.0, 1.0))), "ascending"),
             (dict(spec=raw_spec((0, 2), (1.0, -1.0))), "obs_weight"), (dict(spec=raw_spec((0, 2), (float("nan"), 1.0))), "obs_weight"),
             (dict(spec=raw_spec((), ())), "n_obs"), (dict(spec=raw_spec(tuple(range(65)), (1.0,) * 65)), "n_obs"),
             (dict(spec=spec_of(lam=-0.5), zb=P), "background"), (dict(spec=spec_of(lam=0.5)), "z_background"),
             (dict(spec=spec_of(state=upd(max_norm=1.0))), "state.max_norm"), (dict(spec=spec_of(state=upd(flags=1))), "state.flags"),
             (dict(spec=spec_of(state=upd(flags=8))), "flags"), (dict(spec=spec_of(state=upd(step=0))), "step"),
             (dict(spec=spec_of(state=upd(lr=-1.0))), "lr"), (dict(spec=spec_of(state=upd(size=56))), "size")]
    for kw, word in cases:
        assert step(**kw) == _lib.LNS_EINVAL, kw
        assert word in err(), (kw, err())
    # a missing propagator parameter pointer
    first = next(i for i, (k, _, isb) in enumerate(e.params) if k.startswith("propagator.") and not isb)
    broken = _params(e)
    broken[first] = None
    assert step(params=broken) == _lib.LNS_EINVAL and e.params[first][0] in err()
    # the workspace: the documented layout, and a short one is refused with the needed size in the message
    need = e.fit_step_workspace_bytes(3, lh, lw, 3, 2)
    assert need == e.train_step_workspace_bytes(3, lh, lw, 3) + _round256(8 * 3 * 3) + _round256(4 * 3 * c * lh * lw)
    assert step(nbytes=need - 1) == _lib.LNS_ENOMEM and "workspace" in err() and str(need) in err()
    assert step(ws=None) == _lib.LNS_ENOMEM
    nb = ctypes.c_size_t(0)
    for args in ((0, lh, lw, 3, 2), (3, lh, lw, 0, 2), (3, lh, lw, 3, 0), (3, lh, lw, 3, 65)):
        assert L.lns_fit_step_workspace_bytes(h, *args, ctypes.byref(nb)) == _lib.LNS_EINVAL, args
    assert L.lns_fit_step_workspace_bytes(h, 3, lh, lw, 3, 2, None) == _lib.LNS_EINVAL
    # an engine without a propagator
    ae_only = _engine(prop_kind=_lib.LNS_PROP_NONE)
    assert step(eng=ae_only._h, params=_params(ae_only)) == _lib.LNS_ESTATE and "propagator" in err(ae_only._h)
    assert L.lns_fit_step_workspace_bytes(ae_only._h, 3, lh, lw, 3, 2, ctypes.byref(nb)) == _lib.LNS_ESTATE
    # the conditional propagator: param is required; fitting it needs its three buffers, each spec is checked under its name
    ce = _engine("twophase_cond")
    cp = _params(ce)
    _, ch, cw = ce.latent_shape()

    def cstep(**kw):
        return step(eng=ce._h, params=cp, hh=ch, ww=cw, **kw)
    assert cstep() == _lib.LNS_EINVAL and "param" in err(ce._h)
    both = spec_of(param=True)
    assert cstep(param=P, spec=both) == _lib.LNS_EINVAL and "g_p" in err(ce._h)
    assert cstep(param=P, spec=both, gp=P, mp=P) == _lib.LNS_EINVAL and "exp_avg_sq_p" in err(ce._h)
    assert cstep(param=P, spec=spec_of(param=upd(max_norm=2.0)), gp=P, mp=P, vp=P) == _lib.LNS_EINVAL and "param.max_norm" in err(ce._h)
    assert cstep(param=P, spec=both, gp=P, mp=P, vp=P, nbytes=16) == _lib.LNS_ENOMEM
    assert cstep(param=P, spec=spec_of(state=False, param=True), gz=None, mz=None, vz=None, gp=P, mp=P, vp=P, nbytes=16) == _lib.LNS_ENOMEM


def test_python_front_end_refuses_what_it_cannot_do():
    from lns_amd import config, dropin, engine, fit
    from lns_amd._lib import LnsError
    for bad in ((), (2, 1), (-1, 0), tuple(range(65))):
        with pytest.raises(LnsError):
            engine.normalize_obs(bad)
    with pytest.raises(LnsError):
        engine.normalize_obs((0, 1), (1.0, -1.0))
    m = dropin.build_dynamics(config.preset("ns2d_mini"))
    with pytest.raises(LnsError, match="conditional"):
        fit.LatentFit(m, fit_param=True)
    with pytest.raises(LnsError, match="nothing to fit"):
        fit.LatentFit(m, fit_state=False)
    with pytest.raises(LnsError, match="background"):
        fit.LatentFit(m, background=-1.0)
    assert fit.LatentFit(m).fit_param is False
    with pytest.raises(LnsError, match="no CPU fallback"):
        fit.LatentFit(m).run(torch.zeros(1, 8, 4, 4), torch.zeros(1, 1, 8, 4, 4), [0])


# ---- the reference fit --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setup", lf.TWINS, ids=tr.case_id)
def test_reference_fit_reduces_loss_and_param_error(setup):
    """Float64, 40 Adam iterations from truth + 0.1 N(0,1) (state) and truth + 0.2 (param), observations at steps [0, 2]
    with weights [1, 0.5].  Measured with this reference, worst sample of each setup:
        loss[0] / loss[-1]             E6 7x15 6.9x    E6 2x2 5.8x    E3 4x4 6.8x     asserted: >= 4x
        param error, state + param     E6 7x15 0.2 -> 0.037 (5.4x)    E6 2x2 0.2 -> 0.147 (1.36x)   asserted: >= 4x / 1.2x
        param error, state known       E6 7x15 0.2 -> 0.0216 (9.2x)   E6 2x2 0.2 -> 0.0202 (9.9x)   asserted: >= 7x
        rms state error                falls for every sample (7x15: 0.100 -> 0.076)
    On the 2x2 plane 64 observed numbers face 33 unknowns per sample and one sample's param stays near its start; with the
    state known every param is found.  tests/test_latent_fit_gpu.py asks the engine for at most half of the measured factors
    (latent_fit_reference.GPU_*)."""
    d = lf.twin(setup)
    prop = lf.propagator(setup[0])
    z, p, loss = lf.fit(prop, lf.t64(d["z_start"]), lf.t64(d["p_start"]), lf.t64(d["obs"]), lf.TWIN_STEPS, lf.TWIN_WEIGHTS)
    red = (loss[0] / loss[-1]).numpy()
    print("loss reduction per sample", red)
    assert (red >= lf.CPU_LOSS_RED).all(), red
    rms0 = np.sqrt(((d["z_start"] - d["z_true"]) ** 2).reshape(setup[1], -1).mean(1))
    rms1 = np.sqrt(((z.numpy() - d["z_true"]) ** 2).reshape(setup[1], -1).mean(1))
    print("rms state error", rms0, "->", rms1)
    assert (rms1 < rms0).all()
    if p is not None:
        e1 = np.abs(p.numpy() - d["p_true"])
        print("param error", lf.PARAM_OFFSET, "->", e1)
        assert (e1 <= lf.PARAM_OFFSET / lf.CPU_PARAM_RED[setup]).all(), e1
        _, p1, loss1 = lf.fit(prop, lf.t64(d["z_true"]), lf.t64(d["p_start"]), lf.t64(d["obs"]), lf.TWIN_STEPS, lf.TWIN_WEIGHTS,
                              fit_state=False)
        e2 = np.abs(p1.numpy() - d["p_true"])
        print("param error, state known", lf.PARAM_OFFSET, "->", e2)
        assert (e2 <= lf.PARAM_OFFSET / lf.CPU_PARAM_ONLY_RED).all(), e2


# ---- discrimination and conditioning of the grad_param cases -------------------------------------------------------------
@pytest.mark.parametrize("case", lf.COND_CASES, ids=tr.case_id)
def test_grad_param_inputs_tell_mistakes_from_the_truth(case):
    r64, r32 = lf.adjoint_truth(case)
    truth = lf.grad_param_chain(case)
    # the opened chain is the autograd gradient (float32 trigonometry inside both: agreement to its rounding, not to 1e-16)
    assert tr.rel_l2(truth, r64["grad_param"]) < 1e-6 and tr.rel_max(truth, r64["grad_param"]) < 1e-6
    _, b2, _, bm, _, _ = lf.rule(r64["grad_param"], r64["grad_param"], r32["grad_param"])
    for mistake in lf.MISTAKES:
        wrong = lf.grad_param_chain(case, mistake)
        d2, dm = tr.rel_l2(wrong, truth), tr.rel_max(wrong, truth)
        print(tr.case_id(case), mistake, "rel-L2 %.3g (bound %.3g)  rel-max %.3g (bound %.3g)" % (d2, b2, dm, bm))
        assert d2 >= 100 * b2 and dm >= 100 * bm, (mistake, d2, dm)


@pytest.mark.parametrize("case", lf.ADJOINT_CASES, ids=tr.case_id)
def test_float32_statement_is_well_conditioned(case):
    r64, r32 = lf.adjoint_truth(case)
    for k in ("grad_z0", "grad_param"):
        if r64[k] is None:
            continue
        o2, om = tr.rel_l2(r32[k], r64[k]), tr.rel_max(r32[k], r64[k])
        print(tr.case_id(case), k, "own rel-L2 %.3g rel-max %.3g" % (o2, om))
        assert 3 * o2 <= 1e-3 and 3 * om <= 1e-3, (k, o2, om)


def test_new_kernels_use_no_scratch_and_spill_nothing():
    """tools/kernel_resources.py on the code object: the loss, finish and Fourier-backward kernels have 0 scratch bytes and 0
    spilled registers (memory-bound elementwise / reduction kernels: anything else would be a regression)."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    from lns_amd import _lib
    res = kernel_resources.resources(_lib.LIB_PATH)
    for name in ("obs_mse_kernel", "obs_mse_finish_kernel", "vec_fourier_bwd_kernel"):
        k = [v for n, v in res.items() if name in n]
        assert len(k) == 1, name
        assert k[0]["scratch"] == 0 and k[0]["vgpr_spill"] == 0 and k[0]["sgpr_spill"] == 0 and k[0]["vgpr"] <= 64, (name, k[0])

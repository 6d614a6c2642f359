"""CPU: the host side of the error attribution (include/lns.h "error attribution"): exports and bindings, the refusals of the
entry points (host only, fake pointers), Python argument handling, the float64 identity frame^2 = prop^2 + recon^2 + cross, the
admissibility of the statement's reduction order under the project's rule, the discrimination of the test inputs, and the
resources of the built kernels."""
import ctypes
import os
import sys

import pytest
import torch

import eval_attrib_reference as ar
from helpers import ROOT

NEW = ("lns_rollout_eval_attrib_workspace_bytes", "lns_rollout_eval_attrib", "lns_rollout_latent_eval_attrib",
       "lns_autoencode_eval_workspace_bytes", "lns_autoencode_eval", "lns_op_eval_attrib", "lns_op_latent_err")
FAMILIES = ("unit", "tiny", "huge", "offset")
PLANES = ((3, 5), (17, 16), (23, 29), (61, 121), (128, 128))
FLOOR = 2e-7


def _specs(C, family="unit"):
    """The scalar spec and a per-channel one with walls on channel 0 and the clamp on the last channel.
    The per-channel form subtracts denormalised values, D_c(yhat) - D_c(r), so a mean that dwarfs the family's fluctuation
    flattens every channel in fp32 (0.5 + 3.5e-13 n is 0.5).  The per-channel means are therefore in units of the family's
    fluctuation scale, and the clamp keeps the normalised values between -1 and +1.5 scales around the family's offset: it acts
    on both sides (about 16 % and 7 % of the pixels of a normal field) and leaves three quarters of the channel alone, on
    every family.  (1e3 + 1e-2 x stays hard for this form: x * std is near 2e3, where fp32 resolves 2.4e-4 of differences
    near 2e-3 -- ours and torch's own then share an elementwise error near 1e-3, well above the floor, but neither is 0.)"""
    scale, off = {"unit": (1.0, 0.0), "tiny": (1e-12, 0.0), "huge": (1e12, 0.0), "offset": (1e-2, 1e3)}[family]
    std = [2.1, 1.7, 0.35][:C]
    mean = [m * scale for m in (0.4, -0.2, 0.5)][:C]
    scalar = dict(mean=0.37, std=1.9, eps=1e-8)
    per_ch = dict(mean=mean, std=std, eps=1e-8 * scale * scale, zero_wall_channels=(0,), clamp_channels=(C - 1,),
                  clamp=((off - scale) * std[-1] + mean[-1], (off + 1.5 * scale) * std[-1] + mean[-1]))
    return (("scalar", scalar), ("per_channel", per_ch))


def test_symbols_are_declared_exported_and_bound():
    from lns_amd import _lib, dropin, engine, metrics
    header = open(os.path.join(ROOT, "include", "lns.h")).read()
    L = _lib.lib()
    for sym in NEW:
        assert "int %s(" % sym in header, sym
        assert sym in _lib.SYMBOLS and hasattr(L, sym), sym
        assert getattr(L, sym).argtypes is not None, sym
    assert L.lns_build_has(b"eval_attrib") == 1
    assert '"eval_attrib"' in header and "typedef struct lns_eval_attrib {" in header
    assert ctypes.sizeof(_lib.LnsEvalAttrib) == 8 + 10 * 8 and len(_lib.LnsEvalAttrib.OUTPUTS) == 10
    for name in ("rollout_eval_attrib", "rollout_latent_eval_attrib", "autoencode_eval", "eval_attrib"):
        assert callable(getattr(engine.Engine, name)), name
    assert callable(metrics.error_attribution) and callable(metrics.attribution_shares)
    assert callable(dropin.LatentDynamics.validate_attribution)
    assert callable(dropin.SimpleAutoencoder.validate) and callable(dropin.ConditionalSimpleAutoencoder.validate)
    assert engine.EvalAttrib._fields == ("frame", "seq", "frames", "recon_frame", "recon_seq", "prop_frame", "prop_seq",
                                         "cross_frame", "cross_seq", "latent_frame", "latent_seq", "recon_frames", "z_true")
    assert engine.EvalAttribChunk._fields == engine.EvalAttrib._fields + ("z_last",)
    assert engine.AutoencodeEval._fields == ("frame", "seq", "z")


# ---- refusals (host only) ---------------------------------------------------------------------------------------------
_P = ctypes.c_void_p(0x1000)
_T = 5


def _ints(*v):
    return (ctypes.c_int * len(v))(*v)


def _engines():
    import copy
    from lns_amd import _lib, config, engine
    mini = config.preset("ns2d_mini")
    wide = copy.deepcopy(mini)
    wide.in_channels = 9                                               # above the per-channel form's channel limit
    mk = lambda a, **kw: engine.Engine(engine.make_config(a, ae_prefix="vq_ae.", prop_prefix="propagator.", **kw))
    engines = {"full": mk(mini), "wide": mk(wide), "max4": mk(mini), "noprop": mk(mini, prop_kind=_lib.LNS_PROP_NONE),
               "noprop4": mk(mini, prop_kind=_lib.LNS_PROP_NONE), "noae": mk(mini, ae_kind=_lib.LNS_AE_NONE),
               "cond": engine.Engine(engine.make_config(config.preset("twophase_cond"), ae_prefix="ae.", prop_prefix="propagator.")),
               "condae": engine.Engine(engine.make_config(config.preset("cond_ae_mini"), ae_kind=_lib.LNS_AE_NONSQUARED,
                                                          prop_kind=_lib.LNS_PROP_NONE))}
    engines["max4"].set_option("eval_max_steps", 4)
    engines["noprop4"].set_option("eval_max_steps", 4)
    return engines


def _attrib(size=None, **outputs):
    from lns_amd import _lib
    at = _lib.LnsEvalAttrib()
    at.size = ctypes.sizeof(_lib.LnsEvalAttrib) if size is None else size
    for k, v in outputs.items():
        setattr(at, k, v)
    return at


def _call(L, engines, entry, kw):
    """-> (rc, message or None) of one call; None: the call left the engine's last error alone."""
    from lns_amd import engine
    a = dict(eng="full", start=_P, param=None, y=_P, B=3, T=_T, t0=0, Ttot=_T, spec="ok", frame=_P, seq=_P, k=_ints(0, 3, 4), nk=3,
             frames=_P, at=_attrib(prop_frame=0x1000, recon_frames_out=0x1000), z=_P)
    a.update(kw)
    e = engines[a["eng"]]
    C = e.cfg.in_channels
    sp = engine.eval_spec(min(C, 8), mean=0.37, std=1.9) if a["spec"] != "per_channel" else None
    if sp is None:
        sp = engine.eval_spec(8, mean=[0.1] * 8, std=[1.0] * 8)
    if a["spec"] == "bad":
        sp.size = 8
    assert L.lns_set_option(e._h, b"no such option", 0) != 0           # a known last error: was it replaced?
    mark = L.lns_last_error(e._h)
    spp = ctypes.byref(sp) if a["spec"] is not None else None
    atp = ctypes.byref(a["at"]) if a["at"] is not None else None
    if entry == "lns_rollout_eval_attrib":
        rc = L.lns_rollout_eval_attrib(e._h, a["start"], a["param"], a["y"], a["B"], a["T"], spp, a["frame"], a["seq"], a["k"], a["nk"],
                                       a["frames"], atp, _P, 1 << 40, None)
    elif entry == "lns_rollout_latent_eval_attrib":
        rc = L.lns_rollout_latent_eval_attrib(e._h, a["start"], a["param"], a["y"], a["B"], a["T"], a["t0"], a["Ttot"], spp, a["frame"],
                                              a["seq"], a["k"], a["nk"], a["frames"], None, atp, _P, 1 << 40, None)
    else:
        rc = L.lns_autoencode_eval(e._h, a["start"], a["param"], a["B"], a["T"], spp, a["frame"], a["seq"], a["z"], _P, 1 << 40, None)
    msg = L.lns_last_error(e._h)
    return rc, (None if msg == mark else msg.decode())


_PASSED = (-3, "lns_finalize_weights must be called first")           # every refusal passed: no weights on this machine
_BATCH = (-1, "batch 1073741824 exceeds the maximum of 65535 trajectories per call")
_AT_BAD = (-1, "attrib is null or its size field is not sizeof(lns_eval_attrib)")
_AT_EMPTY = (-1, "attrib: no output is set")
_SPEC = (-1, "spec is null or its size field is not sizeof(lns_eval_spec)")
_MAX = (-1, "5 steps exceed the option eval_max_steps = 4 (it sizes the evaluation workspace)")
_NO_MODEL = (-3, "rollout needs autoencoder and propagator")
_KEEP = (-1, "keep_steps must be ascending steps in [0, 5): entry 2 is 3")
_ROLLOUT_CASES = {
    "valid": (dict(), _PASSED),
    "one_output": (dict(at=_attrib(latent_seq=0x1000)), _PASSED),
    "only_latents": (dict(at=_attrib(z_true_out=0x1000)), _PASSED),
    "no_kept_frames": (dict(k=None, nk=0, frames=None), _PASSED),
    "recon_frames_without_keep": (dict(k=None, nk=0, frames=None, at=_attrib(recon_frames_out=0x1000)), _PASSED),
    "conditional_with_param": (dict(eng="cond", param=_P), _PASSED),
    "attrib_null": (dict(at=None), _AT_BAD),
    "attrib_size": (dict(at=_attrib(size=8, prop_frame=0x1000)), _AT_BAD),
    "attrib_empty": (dict(at=_attrib()), _AT_EMPTY),
    # the existing refusals keep their code, message and place ...
    "start_null": (dict(start=None), (-1, None)),
    "y_null": (dict(y=None), (-1, "y_true is null")),
    "B_0": (dict(B=0), (-1, "B must be positive")),
    "T_0": (dict(T=0, Ttot=0), (-1, "T must be positive")),
    "outputs_null": (dict(frame=None, seq=None), (-1, "frame_out and seq_out are both null")),
    "spec_null": (dict(spec=None), _SPEC),
    "spec_bad": (dict(spec="bad"), _SPEC),
    "per_channel_wide": (dict(eng="wide", spec="per_channel"), (-1, "spec: the per-channel form needs in_channels <= 8")),
    "keep_unsorted": (dict(k=_ints(0, 4, 3)), _KEEP),
    "frames_null": (dict(frames=None), (-1, "frames_out is null but n_keep > 0")),
    "B_huge": (dict(B=1 << 30), _BATCH),
    "past_eval_max_steps": (dict(eng="max4"), _MAX),
    "no_propagator": (dict(eng="noprop"), _NO_MODEL),
    "conditional_without_param": (dict(eng="cond"), (-1, None)),
    # ... and which of two failing checks answers: lns_rollout_eval's arguments, then the attribution's, then the batch, the
    # horizon, the model and param
    "attrib_null+keep_unsorted": (dict(at=None, k=_ints(0, 4, 3)), _KEEP),
    "attrib_null+spec_bad": (dict(at=None, spec="bad"), _SPEC),
    "attrib_size+attrib_empty": (dict(at=_attrib(size=8)), _AT_BAD),
    "attrib_null+B_huge": (dict(at=None, B=1 << 30), _AT_BAD),
    "attrib_empty+past_eval_max_steps": (dict(at=_attrib(), eng="max4"), _AT_EMPTY),
    "attrib_empty+no_propagator": (dict(at=_attrib(), eng="noprop"), _AT_EMPTY),
    "B_huge+no_propagator": (dict(B=1 << 30, eng="noprop"), _BATCH),
}


@pytest.mark.parametrize("entry", ["lns_rollout_eval_attrib", "lns_rollout_latent_eval_attrib"])
def test_refusal_matrix_of_the_attribution_calls(entry):
    from lns_amd import _lib
    L = _lib.lib()
    engines = _engines()
    for name, (kw, (want_rc, want_msg)) in _ROLLOUT_CASES.items():
        rc, msg = _call(L, engines, entry, kw)
        if name == "start_null":
            want_msg = "x is null" if entry == "lns_rollout_eval_attrib" else "z_in is null"
        if name == "conditional_without_param":
            want_msg = "conditional model needs param" if entry == "lns_rollout_eval_attrib" else "conditional propagator needs param"
        assert rc == want_rc, (entry, name, rc, msg)
        assert msg == want_msg, (entry, name, msg)
    # the chunked form: t0 + T against T_total, keep_steps relative to the chunk
    rc, msg = _call(L, engines, "lns_rollout_latent_eval_attrib", dict(T=2, t0=3, k=_ints(0, 1), nk=2))
    assert (rc, msg) == _PASSED
    rc, msg = _call(L, engines, "lns_rollout_latent_eval_attrib", dict(T=3, t0=3, k=_ints(0), nk=1))
    assert (rc, msg) == (-1, "t0 + T = 3 + 3 exceeds T_total = 5 (or t0 < 0)")
    # the size query refuses what lns_rollout_eval_workspace_bytes refuses
    n = ctypes.c_size_t(0)
    for h, B in ((None, 3), (engines["full"]._h, 0), (engines["full"]._h, 1 << 30), (engines["noprop"]._h, 3)):
        assert L.lns_rollout_eval_attrib_workspace_bytes(h, B, ctypes.byref(n)) == L.lns_rollout_eval_workspace_bytes(h, B, ctypes.byref(n)) != 0


_AE_CASES = {
    "valid": (dict(eng="noprop"), _PASSED),
    "with_propagator": (dict(), _PASSED),
    "no_latents": (dict(eng="noprop", z=None), _PASSED),
    "one_output": (dict(eng="noprop", frame=None), _PASSED),
    "conditional_encoder_with_param": (dict(eng="condae", param=_P), _PASSED),
    "x_null": (dict(eng="noprop", start=None), (-1, "x is null")),
    "B_0": (dict(eng="noprop", B=0), (-1, "B must be positive")),
    "T_0": (dict(eng="noprop", T=0), (-1, "T must be positive")),
    "outputs_null": (dict(eng="noprop", frame=None, seq=None), (-1, "frame_out and seq_out are both null")),
    "spec_null": (dict(eng="noprop", spec=None), _SPEC),
    "spec_bad": (dict(eng="noprop", spec="bad"), _SPEC),
    "per_channel_wide": (dict(eng="wide", spec="per_channel"), (-1, "spec: the per-channel form needs in_channels <= 8")),
    "B_huge": (dict(eng="noprop", B=1 << 30), _BATCH),
    "past_eval_max_steps": (dict(eng="noprop4"), _MAX),
    "no_autoencoder": (dict(eng="noae"), (-3, "autoencode_eval needs an autoencoder")),
    "conditional_encoder_without_param": (dict(eng="condae"), (-1, "conditional encoder needs param")),
    "x_null+B_0": (dict(eng="noprop", start=None, B=0), (-1, "x is null")),
    "spec_bad+B_huge": (dict(eng="noprop", spec="bad", B=1 << 30), _SPEC),
    "B_huge+past_eval_max_steps": (dict(eng="noprop4", B=1 << 30), _BATCH),
    "past_eval_max_steps+no_autoencoder": (dict(eng="noae", T=5000), (-1, "5000 steps exceed the option eval_max_steps = 1024 (it sizes the evaluation workspace)")),
}


def test_refusal_matrix_of_autoencode_eval():
    from lns_amd import _lib
    L = _lib.lib()
    engines = _engines()
    for name, (kw, (want_rc, want_msg)) in _AE_CASES.items():
        rc, msg = _call(L, engines, "lns_autoencode_eval", kw)
        assert rc == want_rc, (name, rc, msg)
        assert msg == want_msg, (name, msg)
    n = ctypes.c_size_t(0)
    assert L.lns_autoencode_eval_workspace_bytes(None, 3, ctypes.byref(n)) == _lib.LNS_EINVAL
    assert L.lns_autoencode_eval_workspace_bytes(engines["noprop"]._h, 0, ctypes.byref(n)) == _lib.LNS_EINVAL
    assert L.lns_autoencode_eval_workspace_bytes(engines["noprop"]._h, 1 << 30, ctypes.byref(n)) == _lib.LNS_EINVAL
    assert L.lns_autoencode_eval_workspace_bytes(engines["noae"]._h, 3, ctypes.byref(n)) == _lib.LNS_ESTATE


def test_refusals_of_the_op():
    """Every refusal of lns_op_eval_attrib stands ahead of its first HIP call."""
    from lns_amd import _lib, engine
    L = _lib.lib()
    sp = engine.eval_spec(3, mean=0.37, std=1.9)
    wide = engine.eval_spec(8, mean=[0.1] * 8, std=[1.0] * 8)
    bad = engine.eval_spec(3)
    bad.size = 8
    ok = dict(yhat=_P, r=_P, y=_P, dims=(2, 2, 3, 4, 4), spec=sp, outs=(_P, _P, _P, _P))
    cases = {
        "yhat_null": (dict(yhat=None), "eval_attrib: yhat / r / y is null"),
        "r_null": (dict(r=None), "eval_attrib: yhat / r / y is null"),
        "no_output": (dict(outs=(None,) * 4), "eval_attrib: no output is set"),
        "spec_null": (dict(spec=None), "eval_attrib: spec is null or its size field is not sizeof(lns_eval_spec)"),
        "spec_size": (dict(spec=bad), "eval_attrib: spec is null or its size field is not sizeof(lns_eval_spec)"),
        "T_0": (dict(dims=(2, 0, 3, 4, 4)), "eval_attrib: B, T, C, H, W >= 1, H * W <= 2^30 and B * T * C < 2^31"),
        "planes": (dict(dims=(1 << 15, 1 << 15, 3, 4, 4)), "eval_attrib: B, T, C, H, W >= 1, H * W <= 2^30 and B * T * C < 2^31"),
        "per_channel_wide": (dict(dims=(2, 2, 9, 4, 4), spec=wide), "eval_attrib: the per-channel form needs C <= 8"),
        "r_null+no_output": (dict(r=None, outs=(None,) * 4), "eval_attrib: yhat / r / y is null"),
        "no_output+spec_null": (dict(outs=(None,) * 4, spec=None), "eval_attrib: no output is set"),
    }
    for name, (kw, want) in cases.items():
        a = dict(ok)
        a.update(kw)
        rc = L.lns_op_eval_attrib(a["yhat"], a["r"], a["y"], *a["dims"], ctypes.byref(a["spec"]) if a["spec"] is not None else None,
                                  *a["outs"], None)
        assert rc == _lib.LNS_EINVAL and L.lns_create_error().decode() == want, (name, rc, L.lns_create_error().decode())


def test_python_argument_handling_needs_no_device():
    from lns_amd import metrics
    from lns_amd._lib import LnsError
    engines = _engines()
    x = torch.zeros(2, 3, 32, 32)
    with pytest.raises(LnsError, match="no CPU fallback"):
        engines["full"].rollout_eval_attrib(x, torch.zeros(2, 4, 3, 32, 32))
    with pytest.raises(LnsError, match="no CPU fallback"):
        engines["noprop"].autoencode_eval(torch.zeros(2, 4, 3, 32, 32))
    with pytest.raises(LnsError, match="no CPU fallback"):
        metrics.error_attribution(*(torch.zeros(1, 1, 1, 2, 2),) * 3)
    # the shares of frame^2: plain arithmetic on the result columns, on any device
    prop, recon = torch.tensor([0.3, 0.0]), torch.tensor([0.4, 0.5])
    cross = torch.tensor([0.11, 0.0])
    frame = (prop ** 2 + recon ** 2 + cross).sqrt()
    sp, sr, sc = metrics.attribution_shares(frame, prop, recon, cross)
    assert torch.allclose(sp + sr + sc, torch.ones(2)) and torch.allclose(sp, torch.tensor([0.09 / 0.36, 0.0]))
    assert float(sr[1]) == 1.0 and float(sc[1]) == 0.0


# ---- the statement ----------------------------------------------------------------------------------------------------
ALPHA, BETA = 0.2, 0.02


def _inputs(family, plane, g, C=3, gamma=0.5):
    """alpha, beta: walls leave a 3x5 plane three pixels.  cross / (prop recon) is 2 gamma alpha / sqrt(beta^2 + gamma^2 alpha^2)
    = 1.96 with a relative noise of beta / (|gamma| alpha sqrt(N)) = 0.12 at N = 3, so the sign of gamma and the size 0.1 hold
    on every plane by eight standard deviations; D_c is monotone, so walls and clamp change no pixel's sign of a b."""
    return ar.family(family, (2, 2, C) + plane, g, gamma=gamma, alpha=ALPHA, beta=BETA)


@pytest.mark.parametrize("family", FAMILIES)
def test_float64_statement_satisfies_the_identity_and_the_inputs_are_conditioned(family):
    """frame^2 = prop^2 + recon^2 + cross to 1e-12 relative in float64 on every test input, frame being the relative L2 of the
    forecast formed on its own; and |cross| >= 0.1 prop recon, with the sign of gamma, on every plane under both specs: with y_hat = r + beta n2 + gamma (r - y),
    2 <a, b> = 2 gamma |b|^2 + noise, so cross is no pure cancellation and its relative error means something."""
    g = torch.Generator().manual_seed(11)
    for plane in PLANES:
        for gamma in (0.5, -0.5):
            yh, r, y = _inputs(family, plane, g, gamma=gamma)
            for name, norm in _specs(3, family):
                w = ar.statement64(yh, r, y, **norm)
                for k in ("_frame", "_seq"):
                    lhs, rhs = w["frame" + k] ** 2, w["prop" + k] ** 2 + w["recon" + k] ** 2 + w["cross" + k]
                    assert bool(((lhs - rhs).abs() <= 1e-12 * lhs).all()), (family, plane, gamma, name, k)
                ratio = w["cross_frame"].abs() / (w["prop_frame"] * w["recon_frame"])
                assert float(ratio.min()) >= 0.1, (family, plane, gamma, name, float(ratio.min()))
                assert bool(((w["cross_frame"] > 0) == (gamma > 0)).all()), (family, plane, gamma, name)
                # no column of the fp32 statement is flattened to 0 by the spec: the float64 gates compare numbers, not 0 with 0
                s32 = ar.statement32(yh, r, y, **norm)
                assert all(bool((s32[k] != 0).all()) for k in ar.COLUMNS), (family, plane, gamma, name)


def _rule_ratio(ours, own, want):
    def errs(a):
        d = a.double() - want
        return float(d.abs().max() / want.abs().max()), float(d.norm() / want.norm())
    return max(a / max(FLOOR, 3.0 * b) for a, b in zip(errs(ours), errs(own)))


@pytest.mark.parametrize("family", FAMILIES)
def test_the_statement_is_admissible_under_the_rule(family):
    """The GPU test holds the kernel to max(2e-7, 3 x own) against float64 in both measures.  The statement's reduction order,
    emulated here on the CPU (strided thread sums, pairwise rest; unfused ops), must itself pass that rule on every column with
    torch's CPU reductions as `own`.  The worst ratio ours / bound of each family is printed."""
    g = torch.Generator().manual_seed(5)
    worst = 0.0
    for plane in PLANES:
        for gamma in (0.5, -0.5):
            yh, r, y = _inputs(family, plane, g, gamma=gamma)
            for name, norm in _specs(3, family):
                ours, own, want = ar.statement32(yh, r, y, **norm), ar.statement32_torch(yh, r, y, **norm), ar.statement64(yh, r, y, **norm)
                for k in ar.COLUMNS:
                    ratio = _rule_ratio(ours[k], own[k], want[k])
                    worst = max(worst, ratio)
                    assert ratio <= 1.0, (family, plane, gamma, name, k, ratio)
    print("%s: statement on the CPU / bound = %.3f" % (family, worst))


@pytest.mark.parametrize("mistake", ["r_denominator", "half_cross", "yhat_minus_y", "one_operand", "latent_own_norm"])
def test_the_inputs_discriminate(mistake):
    """Each deliberate mistake moves some column by at least 100 x the bound of the rule on the test inputs (and is therefore
    no identity on them): ||r||^2 as the denominator, cross without its factor 2, (y_hat - y) in place of (y_hat - r), walls /
    clamp applied to one operand only, the latent drift normalised by ||z_t||^2."""
    g = torch.Generator().manual_seed(7)
    yh, r, y = _inputs("unit", (17, 16), g)
    if mistake == "latent_own_norm":
        z_true = torch.randn(3, 5, 4, 4, 4, generator=g)
        z = z_true + 0.3 * torch.randn(3, 5, 4, 4, 4, generator=g) + 0.2 * z_true
        moved = 0.0
        for want, got in zip(ar.latent64(z, z_true), ar.latent64(z, z_true, own_norm=True)):
            assert not torch.equal(want, got)
            moved = max(moved, float((got - want).abs().max() / want.abs().max()))
        assert moved >= 100 * FLOOR, moved                              # (own: fp32 reductions of 64 terms stay below 2e-7 / 3)
        return
    name, norm = _specs(3)[1 if mistake == "one_operand" else 0]
    want, own, got = ar.statement64(yh, r, y, **norm), ar.statement32_torch(yh, r, y, **norm), ar.statement64(yh, r, y, mistake=mistake, **norm)
    moved = 0.0
    for k in ar.COLUMNS:
        d = (got[k] - want[k]).abs().max() / want[k].abs().max()
        o = (own[k].double() - want[k]).abs().max() / want[k].abs().max()
        moved = max(moved, float(d) / max(FLOOR, 3.0 * float(o)))
    assert any(not torch.equal(got[k], want[k]) for k in ar.COLUMNS), mistake
    assert moved >= 100.0, (mistake, moved)


def test_kernels_use_no_scratch_and_spill_nothing():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    from lns_amd import _lib
    res = {k: v for k, v in kernel_resources.resources(_lib.LIB_PATH).items()
           if any(n in k for n in ("attrib_group_kernel", "latent_err_group_kernel", "attrib_finish_kernel"))}
    assert len(res) == 3, sorted(res)
    for name, r in res.items():
        print(name, r)
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
        assert r["lds"] <= 64, (name, r)                               # the eight reduction slots
        assert r["vgpr"] + r["agpr"] <= 64, (name, r)                   # 256 threads: eight blocks per CU fit the register file

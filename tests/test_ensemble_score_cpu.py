"""CPU: the ensemble validation (lns_rollout_latent_ensemble_eval, lns_op_ensemble_score, include/lns.h) is declared,
exported and bound, refuses bad arguments before any device work in the documented order, its two kernels use no scratch
memory -- and the float64 reference the GPU tests hold it to (tests/ensemble_score_reference.py) has the properties a
CRPS / spread / rank reference must have."""
import ctypes
import os
import re
import sys

import pytest

from helpers import ROOT

SCORE_SYMBOLS = ("lns_rollout_latent_ensemble_eval", "lns_op_ensemble_score")
_P = ctypes.c_void_p(0x1000)                          # stands for a device pointer; never dereferenced
_T = 5


def _ints(*v):
    return (ctypes.c_int * len(v))(*v)


def _spec(size=None, per_channel=0):
    from lns_amd import _lib
    s = _lib.LnsEvalSpec()
    s.size = ctypes.sizeof(_lib.LnsEvalSpec) if size is None else size
    s.per_channel = per_channel
    s.mean, s.std, s.eps = 0.0, 1.0, 1e-8
    return s


def test_score_symbols_are_declared_exported_and_bound():
    from lns_amd import _lib, dropin, engine, metrics
    _lib.build()
    src = open(os.path.join(ROOT, "include", "lns.h")).read()
    assert "w = w + |v_m - v_n|" in src and "the fair CRPS" in src          # the statement is in the header
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(lns_[a-z0-9_]+)\s*\(", src))
    L = ctypes.CDLL(_lib.LIB_PATH)
    for s in SCORE_SYMBOLS:
        assert s in declared, "not declared in include/lns.h: " + s
        assert hasattr(L, s), "missing export: " + s
        assert s in _lib.SYMBOLS
        assert getattr(_lib.lib(), s).argtypes, "not bound in _lib.lib(): " + s
    assert re.search(r"#define\s+LNS_ABI_VERSION\s+2\b", src)         # additive: the ABI version stays
    assert _lib.lib().lns_build_has(b"ensemble_score") == 1
    assert _lib.lib().lns_build_has(b"rollout_ensemble") == 1
    assert engine.EnsembleScores._fields == ("rel_l2", "rmse", "spread", "crps", "seq", "rank", "mean", "var", "z_last")
    for owner, name in ((engine.Engine, "ensemble_score"), (engine.Engine, "rollout_latent_ensemble_eval"),
                        (dropin.LatentDynamics, "validate_ensemble"), (metrics, "spread_skill_ratio")):
        assert callable(getattr(owner, name))


def _engines():
    from lns_amd import _lib, config, engine
    mini = config.preset("ns2d_mini")
    return {"full": engine.Engine(engine.make_config(mini, ae_prefix="vq_ae.", prop_prefix="propagator.")),
            "cond": engine.Engine(engine.make_config(config.preset("twophase_cond"), ae_prefix="ae.", prop_prefix="propagator.")),
            "noprop": engine.Engine(engine.make_config(mini, prop_kind=_lib.LNS_PROP_NONE, ae_prefix="vq_ae."))}


_PASSED = (-3, "lns_finalize_weights must be called first")        # every refusal passed: no weights on this machine
_BATCH = (-1, "batch 65536 exceeds the maximum of 65535 trajectories per call")
_NO_MODEL = (-3, "rollout needs autoencoder and propagator")
_KEEP_2_3 = (-1, "keep_steps must be ascending steps in [0, 5): entry 2 is 3")
_N_KEEP_1 = (-1, "n_keep must be at least 1 (for no decoded step: lns_rollout with to_x = 0)")
_B, _M, _T0 = (-1, "B must be positive"), (-1, "M must be positive"), (-1, "T must be positive")
_Y, _S = (-1, "y_true is null"), (-1, "scores_out is null")
_MR = (-1, "ensemble scoring needs M in 2 .. 128")
_VM = (-1, "var_out needs mean_out")
_SPEC = (-1, "spec is null or its size field is not sizeof(lns_eval_spec)")
# (arguments of the call that differ from a valid one, expected (return code, message))
_REFUSALS = [
    (dict(), _PASSED), (dict(seq=None, rank=None, mean=None, var=None), _PASSED), (dict(var=None), _PASSED),
    (dict(last=_P), _PASSED), (dict(param=_P), _PASSED), (dict(ws=None), _PASSED), (dict(M=2), _PASSED), (dict(M=128), _PASSED),
    (dict(B=511, M=128), _PASSED), (dict(spec="per_channel"), _PASSED),
    (dict(z=None), (-1, "z_in is null")), (dict(y=None), _Y), (dict(scores=None), _S),
    (dict(B=0), _B), (dict(B=-1), _B), (dict(M=0), _M), (dict(M=-1), _M), (dict(T=0), _T0), (dict(T=-1), _T0),
    (dict(M=1, var=None), _MR), (dict(M=129), _MR), (dict(M=1), (-1, "var_out needs M >= 2")),
    (dict(mean=None), _VM),
    (dict(spec=None), _SPEC), (dict(spec="short"), _SPEC),
    (dict(k=_ints(0, 4, 3)), _KEEP_2_3), (dict(k=None), (-1, "keep_steps is null")),
    (dict(nk=0), _N_KEEP_1), (dict(nk=-1), _N_KEEP_1),
    (dict(B=512, M=128), _BATCH),
    (dict(eng="noprop"), _NO_MODEL),
    (dict(eng="cond"), (-1, "conditional propagator needs param")), (dict(eng="cond", param=_P), _PASSED),
    # two failing checks: arguments (in the order of the list above), then the batch, then the model, then param
    (dict(z=None, y=None), (-1, "z_in is null")), (dict(y=None, scores=None), _Y), (dict(scores=None, B=0), _S),
    (dict(B=0, M=0), _B), (dict(M=0, T=0), _M), (dict(T=0, M=129), _T0), (dict(M=129, mean=None), _MR),
    (dict(mean=None, spec=None), _VM), (dict(spec=None, nk=0), _SPEC), (dict(nk=0, k=None), _N_KEEP_1),
    (dict(k=_ints(0, 4, 3), B=512, M=128), _KEEP_2_3), (dict(spec=None, B=512, M=128), _SPEC),
    (dict(y=None, eng="noprop"), _Y), (dict(B=512, M=128, eng="noprop"), _BATCH),
    (dict(B=512, M=128, eng="cond"), _BATCH), (dict(M=129, eng="cond"), _MR), (dict(eng="noprop", param=_P), _NO_MODEL),
]


def test_ensemble_eval_refuses_bad_arguments_without_a_device():
    """Every refusal is decided before the first HIP call (fake pointers, no device here), in the order arguments, batch
    (on B * M), model, param; a call that passes them all stops at the weights that were never finalised."""
    from lns_amd import _lib
    L = _lib.lib()
    engines = _engines()
    specs = {"ok": _spec(), "short": _spec(size=8), "per_channel": _spec(per_channel=1)}
    assert L.lns_rollout_latent_ensemble_eval(None, _P, None, _P, 2, 3, _T, _ints(0, 3, 4), 3, ctypes.byref(specs["ok"]), _P, _P, _P,
                                              _P, _P, None, _P, 1 << 30, None) == _lib.LNS_EINVAL
    for kw, (want_rc, want_msg) in _REFUSALS:
        a = dict(eng="full", z=_P, param=None, y=_P, B=2, M=3, T=_T, k=_ints(0, 3, 4), nk=3, spec="ok", scores=_P, seq=_P, rank=_P,
                 mean=_P, var=_P, last=None, ws=_P)
        a.update(kw)
        h = engines[a["eng"]]._h
        sp = ctypes.byref(specs[a["spec"]]) if a["spec"] else None
        rc = L.lns_rollout_latent_ensemble_eval(h, a["z"], a["param"], a["y"], a["B"], a["M"], a["T"], a["k"], a["nk"], sp, a["scores"],
                                                a["seq"], a["rank"], a["mean"], a["var"], a["last"], a["ws"], 1 << 30, None)
        assert (rc, L.lns_last_error(h).decode()) == (want_rc, want_msg), kw


def test_ensemble_score_op_refuses_bad_arguments_without_a_device():
    from lns_amd import _lib
    L = _lib.lib()
    ok, short, per_c = _spec(), _spec(size=8), _spec(per_channel=1)

    def op(frames=_P, y=_P, n=2, B=2, M=3, C=3, H=4, W=5, spec=ok, scores=_P):
        return L.lns_op_ensemble_score(frames, y, n, B, M, C, H, W, ctypes.byref(spec) if spec is not None else None, scores, _P, _P,
                                       None, None)
    for kw, word in ((dict(frames=None), "null"), (dict(y=None), "null"), (dict(scores=None), "null"), (dict(spec=None), "spec is null"),
                     (dict(spec=short), "spec is null"), (dict(M=1), "M in 2 .. 128"), (dict(M=129), "M in 2 .. 128"), (dict(M=0), "M in 2"),
                     (dict(n=0), "n >= 1"), (dict(B=0), "B in"), (dict(B=65536), "B in"), (dict(C=0), "C, H, W"), (dict(H=0), "C, H, W"),
                     (dict(W=-1), "C, H, W"), (dict(H=1 << 16, W=1 << 15), "H * W"), (dict(n=1 << 16, B=1 << 15, C=8), "n * B * C"),
                     (dict(C=9, spec=per_c), "C <= 8")):
        assert op(**kw) == _lib.LNS_EINVAL, kw
        assert word in L.lns_create_error().decode(), (kw, L.lns_create_error())


def test_score_kernels_use_no_scratch_and_spill_nothing():
    """tools/kernel_resources.py on the code object: 0 scratch bytes and 0 spilled registers for the scoring kernel (its
    member values live in LDS, not in a register array) and its finish kernel."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    from lns_amd import _lib
    res = kernel_resources.resources(_lib.LIB_PATH)
    for name in ("ensemble_score_kernel", "ensemble_score_finish_kernel"):
        k = [v for n, v in res.items() if name in n]
        assert len(k) == 1, name
        assert k[0]["scratch"] == 0 and k[0]["vgpr_spill"] == 0 and k[0]["sgpr_spill"] == 0, (name, k[0])


# ---- the reference itself (float64, CPU) ----------------------------------------------------------------------------------
torch = pytest.importorskip("torch")


def _fields(n, B, M, C, H, W, seed, scale=1.0):
    g = torch.Generator()
    g.manual_seed(seed)
    frames = torch.randn((n, B, M, C, H, W), generator=g) * scale
    y = torch.randn((B, n, C, H, W), generator=g) * scale
    return frames, y


def test_reference_pair_sum_is_the_sorted_form():
    import ensemble_score_reference as ref
    for M in (2, 3, 7, 33):
        v = torch.randn((M, 50), dtype=torch.float64, generator=torch.Generator().manual_seed(M))
        pairs = sum((v[m] - v[n]).abs() for m in range(M - 1) for n in range(m + 1, M))
        assert torch.allclose(ref.pair_sum_sorted(v), pairs, rtol=1e-13, atol=1e-13)
        # and the explicit fp32 statement agrees with the float64 outputs to fp32 rounding
        frames, y = _fields(2, 2, M, 2, 3, 5, M)
        mu, var, crps, rank = ref.statement32(frames, y, mean=0.25, std=1.5)
        r = ref.scores64(frames, y, mean=0.25, std=1.5)
        for a, b in ((mu, r["mu"]), (var, r["var"]), (crps, r["crps"])):
            assert float((a.double() - b).abs().max()) <= 2e-5 * max(1.0, float(b.abs().max()))
        assert torch.equal(ref.rank_histogram(rank, M), r["rank"])


def test_reference_degenerate_ensembles():
    import ensemble_score_reference as ref
    n, B, M, C, H, W = 2, 2, 5, 2, 3, 4
    frames, y = _fields(n, B, M, C, H, W, 3)
    # rounded to bfloat16 (8 significant bits): every partial sum k * v, k <= 5, is exact in fp32, so the fp32 mean is v itself
    same = frames[:, :, :1].to(torch.bfloat16).to(torch.float32).expand(n, B, M, C, H, W).contiguous()
    r = ref.scores64(same, y)
    q = y.double().permute(1, 0, 2, 3, 4)
    assert float(r["var"].abs().max()) == 0.0
    assert torch.allclose(r["crps"], (same[:, :, 0].double() - q).abs(), rtol=0, atol=1e-15)      # w = 0: crps = |v - q|
    assert float(r["scores"][..., 2].abs().max()) == 0.0                                           # spread
    mu32, var32, crps32, _ = ref.statement32(same, y)
    assert torch.equal(mu32, same[:, :, 0]) and float(var32.abs().max()) == 0.0
    assert torch.allclose(crps32, (same[:, :, 0] - y.permute(1, 0, 2, 3, 4)).abs(), rtol=1e-6, atol=0)   # a = 5 rounded additions, / 5
    # M = 2 with the truth between the members: a / 2 = |v0 - v1| / 2 = w / 2
    lo, hi = torch.full((1, 1, 1, 1, 2, 2), -1.0), torch.full((1, 1, 1, 1, 2, 2), 3.0)
    two = torch.cat([lo, hi], 2)
    inside = torch.tensor([-1.0, 0.0, 2.5, 3.0]).view(1, 1, 1, 2, 2)
    r2 = ref.scores64(two, inside)
    assert float(r2["crps"].abs().max()) == 0.0
    assert float(ref.statement32(two, inside)[2].abs().max()) == 0.0


def test_reference_ranks_and_scaling():
    import ensemble_score_reference as ref
    n, B, M, C, H, W = 2, 3, 7, 2, 5, 6
    frames, y = _fields(n, B, M, C, H, W, 9)
    r = ref.scores64(frames, y, eps=1e-30)
    assert r["rank"].shape == (B, n, C, M + 1) and bool((r["rank"].sum(-1) == H * W).all())
    assert bool((r["scores"][..., 1:] >= 0).all()) and bool((r["crps"] >= -1e-15).all())
    # a power of two scales crps, rmse and spread and leaves rel_l2 and the ranks alone -- exactly, in float64 and in the fp32 statement
    s = ref.scores64(frames * 8.0, y * 8.0, eps=1e-30)
    assert torch.equal(s["scores"][..., 1:], r["scores"][..., 1:] * 8.0) and torch.equal(s["seq"][..., 1:], r["seq"][..., 1:] * 8.0)
    assert torch.equal(s["scores"][..., 0], r["scores"][..., 0]) and torch.equal(s["seq"][..., 0], r["seq"][..., 0])
    assert torch.equal(s["rank"], r["rank"])
    a, b = ref.statement32(frames, y), ref.statement32(frames * 8.0, y * 8.0)
    assert torch.equal(b[0], a[0] * 8.0) and torch.equal(b[1], a[1] * 64.0) and torch.equal(b[2], a[2] * 8.0) and torch.equal(b[3], a[3])
    # torch's own fp32 reductions land on the float64 values to fp32 rounding
    own = ref.scores32_torch(frames, y, eps=1e-30)
    assert float((own["scores"].double() - r["scores"]).abs().max()) <= 1e-5 * float(r["scores"].abs().max())


def test_reference_denormalisation_forms():
    import ensemble_score_reference as ref
    x = torch.randn((2, 3, 4, 5), generator=torch.Generator().manual_seed(1))
    assert torch.equal(ref.denorm(x, dict(mean=0.5, std=2.0)), x * 2.0 + 0.5)
    v = ref.denorm(x, dict(mean=[0.0, 1.0, 0.5], std=[1.0, 2.0, 3.0], zero_wall_channels=(0,), clamp_channels=(2,), clamp=(0.0, 1.0)))
    assert float(v[:, 0, 0].abs().max()) == 0.0 and float(v[:, 0, :, -1].abs().max()) == 0.0
    assert torch.equal(v[:, 0, 1:-1, 1:-1], x[:, 0, 1:-1, 1:-1]) and torch.equal(v[:, 1], x[:, 1] * 2.0 + 1.0)
    assert torch.equal(v[:, 2], (x[:, 2] * 3.0 + 0.5).clamp(0.0, 1.0))

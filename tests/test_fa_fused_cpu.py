"""CPU: lns_op_fa_fused's argument checks (they precede the first HIP call, so they need no device), and the case grid of
tests/fa_fused_reference.py: it holds every class it has to hold, its inputs lie inside the design's full-accuracy domain
(the documented two-term arithmetic, `model`, stays below a third of KERNEL_TOL on every plane outside the RELAXED families),
and it would catch a subtly wrong kernel: twelve deliberate mistakes applied to the float64 statement each exceed 10 x the
bound the GPU test holds the kernels to, on at least one plane of at least one case."""
import ctypes

import numpy as np
import pytest

import fa_fused_reference as fr

NAMES = [c["name"] for c in fr.GRID]


def _refusal_args(**over):
    """Arguments of a 64 x 64 call that passes every check; the pointers are host memory no check dereferences."""
    from lns_amd import _lib
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    a = _lib.LnsFaFusedArgs()
    a.x, a.x_bs, a.ss, a.bound, a.w_host, a.kx, a.ky = p, 64 * 64 * 64, None, 1.0, p, p, p
    a.B, a.heads, a.dim_head, a.Cin, a.H, a.W, a.eps, a.instnorm, a.form, a.gpb, a.b_rev = 1, 1, 16, 64, 64, 64, 1e-5, 1, 0, 0, 0
    a.out, a.amax_out = p, None
    for k, v in over.items():
        setattr(a, k, v)
    return a, buf


REFUSALS = [
    dict(x=None), dict(w_host=None), dict(kx=None), dict(ky=None), dict(out=None),
    dict(B=0), dict(B=-3), dict(heads=0),
    dict(H=48, W=48, Cin=96, dim_head=24, x_bs=48 * 48 * 96), dict(Cin=128, x_bs=64 * 64 * 128), dict(dim_head=24), dict(dim_head=0),
    dict(H=32), dict(H=32, W=32, Cin=32, x_bs=32 * 32 * 32),
    dict(dim_head=48, gpb=2), dict(dim_head=64, gpb=3), dict(dim_head=32, gpb=4), dict(gpb=-1),
    dict(form=3), dict(form=-1), dict(H=32, W=32, x_bs=32 * 32 * 64, form=1), dict(H=32, W=32, Cin=128, x_bs=32 * 32 * 128, form=2),
    dict(bound=0.0), dict(bound=-1.0), dict(bound=float("nan")),
    dict(x_bs=64 * 64 * 64 - 1), dict(x_bs=0),
]


def test_build_advertises_the_entry_point():
    from lns_amd import _lib
    L = _lib.lib()
    assert L.lns_build_has(b"op_fa_fused") == 1
    assert L.lns_op_fa_fused(None, None) == _lib.LNS_EINVAL and L.lns_create_error().startswith(b"fa_fused: ")


@pytest.mark.parametrize("over", REFUSALS, ids=lambda d: ",".join("%s=%s" % kv for kv in d.items()))
def test_refusals_precede_the_first_hip_call(over):
    """LNS_EINVAL with the message prefix.  Without a device a call that got past its checks returns LNS_EHIP instead, with
    one a launch on these host pointers would: no refusal reaches a launch."""
    from lns_amd import _lib
    L = _lib.lib()
    a, keep = _refusal_args(**over)
    assert L.lns_op_fa_fused(ctypes.byref(a), None) == _lib.LNS_EINVAL, over
    assert L.lns_create_error().startswith(b"fa_fused: "), L.lns_create_error()


def test_grid_covers_every_class():
    """Every value of every case dimension appears with every kernel."""
    for kern in fr.KERNELS:
        cs = [c for c in fr.GRID if c["kern"] == kern]
        assert {c["dh"] for c in cs} == {16, 32, 48, 64}, kern
        assert {c["heads"] for c in cs} == {1, 2, 3}, kern
        assert {c["B"] for c in cs} == {1, 3, 8, 9}, kern
        assert {(c["dh"], c["gpb"]) for c in cs} == set(fr.DIM_GPB), kern
        assert {(dh, g) for dh, g in fr.DIM_GPB if g} == {(dh, g) for dh in (16, 32, 48, 64) for g in (1, 2, 3, 4) if (dh // 16) % g == 0}
        assert {fr.gpb_of(c) for c in cs} == {1, 2, 3, 4}, kern
        for key in ("b_rev", "instnorm", "strided", "ss_null", "tight"):
            assert {int(c[key]) for c in cs} == {0, 1}, (kern, key)
        assert {c["kind"] for c in cs} == set(fr.KINDS), kern
        assert {c["instnorm"] for c in cs if c["kind"] == "eps_regime"} == {1}
        assert not any(c["tight"] for c in cs if c["kind"].startswith("quiet"))        # the planner's bound: the domain's statement
        assert not any(c["ss_null"] for c in cs if c["kind"] in fr.NEEDS_SS)
    assert {c["instnorm"] for c in fr.GRID if c["kind"] == "zero_row"} == {0, 1}
    assert {(c["B"] & 7) == 0 for c in fr.GRID if c["b_rev"]} == {False, True}          # both block-to-sample maps, reversed
    big = max(fr.GRID, key=lambda c: c["B"] * c["heads"] * c["dh"] * c["H"] * c["W"])
    assert (big["kern"], big["B"], big["heads"], big["dh"]) == ("b0", 9, 2, 64)
    assert 2 * sum(c["heads"] == 1 for c in fr.GRID) > len(fr.GRID)                    # most cases: one head


@pytest.mark.parametrize("name", NAMES)
def test_inputs_are_what_the_family_says(name):
    r = fr.reference(name)
    case, inp = r["case"], r["inp"]
    assert np.isfinite(r["ref"]).all()
    assert (inp["amax"] > 0).all() and inp["amax"].max() <= inp["bound"]
    if case["kind"] == "eps_regime":
        v = fr.statement64(dict(case, instnorm=0), inp).var(axis=(2, 3))
        assert 1e-6 < v.min() and v.max() < 1e-4, (v.min(), v.max())
    if case["kind"] == "zero_row":
        assert not r["ref"][:, fr.zero_plane(case)].any()
    if case["kind"] == "sample_scales":
        assert inp["amax"].max() / inp["amax"].min() > 1e4
    if case["kind"] == "heavy_w":
        rows = np.abs(inp["w"]).sum(axis=1)
        assert rows.max() > 20 * np.median(np.abs(inp["w"]))


@pytest.mark.parametrize("name", NAMES)
def test_model_says_the_case_is_inside_the_domain(name):
    r = fr.reference(name)
    for k, measure in enumerate(("rel-L2", "rel-max")):
        assert r["rounded"][k].max() < 0.1 * fr.KERNEL_TOL, (name, measure, r["rounded"][k].max())
        if not fr.relaxed(r["case"]):
            assert r["model"][k].max() < fr.KERNEL_TOL / 3, (name, measure, r["model"][k].max())
        assert (r["bounds"][k] >= fr.KERNEL_TOL).all() and np.isfinite(r["bounds"][k]).all()


def test_model_locates_the_edge_of_the_domain():
    """quiet_channel(r): the model's error of the planes that read the quiet channel alone grows as its low fp16 term runs out
    of bits -- inside KERNEL_TOL / 3 down to r = 2^-8, beyond KERNEL_TOL from 2^-12."""
    for k in fr.QUIET:
        worst = max(fr.reference(c["name"])["model"][0][:, fr.quiet_planes(c)].max() for c in fr.GRID if c["kind"] == "quiet%d" % k)
        print("quiet_channel(2^-%d): model rel-L2 of the quiet planes %.2e" % (k, worst))
        assert (worst < fr.KERNEL_TOL / 3) == (k <= 8) and (worst > fr.KERNEL_TOL) == (k >= 12), (k, worst)


@pytest.mark.parametrize("mistake", fr.MISTAKES)
def test_mistake_is_caught(mistake):
    worst = {}
    for c in fr.GRID:
        r = fr.reference(c["name"])
        e = fr.plane_errors(fr.statement64(c, r["inp"], mistake), r["ref"])
        worst[c["name"]] = max(float((x / b).max()) for x, b in zip(e, r["bounds"]))
    top = max(worst, key=worst.get)
    caught = [n for n, v in worst.items() if v > 10.0]
    print("%s: %d of %d cases beyond 10 x the bound; largest %.3g x at %s" % (mistake, len(caught), len(worst), worst[top], top))
    assert worst[top] > 10.0, (mistake, top, worst[top])
    if mistake == "p_times_2":
        # InstanceNorm hides a scale unless the plane variance is near eps: every raw and every eps_regime case sees it (and the
        # quiet sample / the quiet planes of sample_scales and quiet_channel), no normalised plain or heavy_w case does
        for c in fr.GRID:
            if not c["instnorm"] or c["kind"] == "eps_regime":
                assert c["name"] in caught, c["name"]
            elif c["kind"] in ("plain", "heavy_w", "heavy_k"):
                assert worst[c["name"]] < 10.0, (c["name"], worst[c["name"]])


def test_float64_fablock_agrees_with_the_float32_oracle():
    """fa_block64 (what tests/test_fa_fused_gpu.py holds a plan's FABlock to) against the float32 CPU oracle's fa_block, on the
    two decoder FABlocks of ns2d_128 at a small non-square plane: STAGE_TOL, the project's tolerance against the oracle."""
    import lns_oracle
    from helpers import rel_l2, synthetic_state_dict
    from lns_amd import config, dropin, filler
    args = config.preset("ns2d_128")
    shapes = {k: tuple(v.shape) for k, v in dropin.build_dynamics(args).state_dict().items()}
    sd = synthetic_state_dict(shapes, 1)
    net = lns_oracle.OracleDynamics(args, sd).ae.net
    blocks = [k[:-len(".in_proj.weight")] for k in sd if k.endswith(".in_proj.weight") and ".decoder." in k]
    assert len(blocks) == 2
    for p in blocks:
        x = filler.normal("blk" + p, (2, sd[p + ".in_proj.weight"].shape[1], 16, 24), 3)
        ref = lns_oracle.fa_block(net, x, p, args.attn_heads)
        out, ops = fr.fa_block64(sd, p, x, args.attn_heads)
        e, ed = rel_l2(out.astype(np.float32), ref), rel_l2((out - x).astype(np.float32), ref - x)
        print("%s: float64 block against the float32 oracle %.2e (its change of the input alone %.2e)" % (p, e, ed))
        assert e < 2e-5 and ed < 2e-5
        assert ops["kx"].shape == (2, args.attn_heads, 16, 16) and ops["ky"].shape == (2, args.attn_heads, 24, 24)

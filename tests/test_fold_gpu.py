"""GPU (-m gpu): adjacent linear convolutions run as ONE convolution on weights composed at pack time ("fold_linear",
csrc/lns_fold.h; DESIGN.md "Folded linear pairs") -- against the CPU oracle and against the pair as it ran before
(fold_linear = 0: the fused 64 -> 64 epilogue of ns2d_64's output layer, two launches in ns2d_mini).

Tolerances.  STAGE_TOL (tests/test_gpu_parity.py) for a whole encode / decode against the oracle.  Between the two arms
2e-6 relative L2, the op-level tolerance the project holds its convolution kernels to: the arms differ by the rounding
of two convolutions' worth of fp32 / split-operand arithmetic at two places of the decoder (3.4e-7 for the output layer
alone in fp32 on the CPU), not by anything that grows with depth -- everything between the two places is the same code
on inputs that differ by that much."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from helpers import rel_l2  # noqa: E402

pytestmark = pytest.mark.gpu

B = 2
STAGE_TOL = 2e-5
ARM_TOL = 2e-6

_cases = {}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _case(name):
    """(args, model, oracle, x, oracle latent z_ref, oracle decode of z_ref) -- built once per preset, never written."""
    if name not in _cases:
        import gpu_checks as gc
        from lns_amd import config, filler
        args = config.preset(name)
        model, orc = gc.build_models(args, 1)
        x = filler.normal("x", (B, args.in_channels, args.Ly, args.Lx), 7)
        z_ref = orc.x_to_z(x)
        y_ref = orc.z_to_x(z_ref)
        _cases[name] = (args, model, orc, x, z_ref, y_ref)
    return _cases[name]


def _decode(eng, zd, fold):
    eng.set_option("fold_linear", fold)
    y = eng.decode(zd)
    torch.cuda.synchronize()
    return y.cpu().numpy()


@pytest.mark.parametrize("name", ["ns2d_64", "ns2d_mini"])
def test_folded_and_unfolded_decode_match_oracle_and_each_other(name):
    _need_gpu()
    args, model, orc, x, z_ref, y_ref = _case(name)
    zd = torch.from_numpy(z_ref).cuda()
    eng = model._engine(zd)
    try:
        y_on = _decode(eng, zd, 1)
        y_off = _decode(eng, zd, 0)
        e_on, e_off, e_arms = rel_l2(y_on, y_ref), rel_l2(y_off, y_ref), rel_l2(y_on, y_off)
        print("%s decode B=%d: fold on vs oracle %.3e, fold off vs oracle %.3e, on vs off %.3e" % (name, B, e_on, e_off, e_arms))
        assert np.isfinite(y_on).all() and np.isfinite(y_off).all()
        assert e_on < STAGE_TOL and e_off < STAGE_TOL, (e_on, e_off)
        assert e_arms < ARM_TOL, e_arms
        if name == "ns2d_mini":                                    # the encoder's last 1x1 -> quant_conv, folded
            eng.set_option("fold_linear", 1)
            z = eng.encode(torch.from_numpy(x).cuda())
            torch.cuda.synchronize()
            e_z = rel_l2(z.cpu().numpy(), z_ref)
            print("%s encode B=%d: fold on vs oracle %.3e" % (name, B, e_z))
            assert e_z < STAGE_TOL, e_z
    finally:
        eng.set_option("fold_linear", 1)


def _forms(eng, zd, fold):
    eng.set_option("fold_linear", fold)
    eng.timing_enable(True)
    eng.decode(zd)
    torch.cuda.synchronize()
    t = eng.timing()
    eng.timing_enable(False)
    return {k: v["launches"] for k, v in t.items()}


def test_plan_has_no_fused_epilogue_and_one_1x1_launch_fewer():
    """ns2d_64: with the fold on no 3x3 form carries the "+ fused 1x1" epilogue (the off arm's output layer does), and the
    decoder's head -- post_quant_conv -> decoder.model.0 -- is one launch instead of two: the 1x1 class has one launch fewer.

    Which FORM loses the launch: off, post_quant_conv reads the caller's latent (no activation bound: fp32 MFMA) and
    decoder.model.0 reads its output (bounded: the f16x2 input-stationary form); on, the composed 16 -> 128 conv reads the
    caller's latent, so the fp32-MFMA form keeps its one launch and the f16x2 form loses one.  (In a rocprofv3 trace the
    16-cout fp32 instantiation loses a launch per step and the 64-cout-tile fp32 one gains it.)"""
    _need_gpu()
    args, model, orc, x, z_ref, y_ref = _case("ns2d_64")
    zd = torch.from_numpy(z_ref).cuda()
    eng = model._engine(zd)
    try:
        on, off = _forms(eng, zd, 1), _forms(eng, zd, 0)
        print("fold on :", sorted(on.items()))
        print("fold off:", sorted(off.items()))
        fused = lambda t: [k for k in t if k.startswith("conv3x3") and "+ fused 1x1" in k]   # noqa: E731
        assert fused(off), off
        assert not fused(on), on
        c3 = [k for k in off if k.startswith("conv3x3") and "/" not in k]
        c1 = [k for k in off if k.startswith("conv1x1") and "/" not in k]
        assert len(c3) == 1 and len(c1) == 1, off
        assert on[c3[0]] == off[c3[0]], (on, off)                  # the output layer is one launch in both arms
        assert on[c1[0]] == off[c1[0]] - 1, (on, off)              # the head is one launch instead of two
        f32 = [k for k in off if k.startswith("conv1x1") and k.endswith("/fp32 MFMA 1x1")]
        assert len(f32) == 1 and on.get(f32[0], 0) == off[f32[0]] == 1, (on, off)
        others = {k: v for k, v in off.items() if not k.startswith("conv")}
        assert others == {k: v for k, v in on.items() if not k.startswith("conv")}
    finally:
        eng.timing_enable(False)
        eng.set_option("fold_linear", 1)


def test_reloaded_weights_recompose_the_folded_packs():
    """A second state_dict loaded into a model that has already run decodes bit for bit like a fresh model built from it:
    the composed weights are rebuilt by every weight load, not kept from the first one."""
    _need_gpu()
    import gpu_checks as gc
    from helpers import synthetic_state_dict
    args, model0, orc, x, z_ref, y_ref = _case("ns2d_mini")
    zd = torch.from_numpy(z_ref).cuda()
    used, _ = gc.build_models(args, 1)                             # (its own model: the shared case is never written)
    y_first = used._engine(zd).decode(zd)
    torch.cuda.synchronize()
    shapes = {k: tuple(v.shape) for k, v in used.state_dict().items()}
    sd2 = synthetic_state_dict(shapes, 2)
    used.load_state_dict({k: torch.from_numpy(v) for k, v in sd2.items()}, strict=True)
    y_reload = used._engine(zd).decode(zd)
    fresh, _ = gc.build_models(args, 2)
    y_fresh = fresh._engine(zd).decode(zd)
    torch.cuda.synchronize()
    assert not torch.equal(y_first, y_reload)
    assert torch.equal(y_reload.view(torch.int32), y_fresh.view(torch.int32))

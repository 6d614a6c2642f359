"""GPU (-m gpu): FABlock2D pools its normalised input and never runs the full-resolution to_in convolution (DESIGN.md
"FABlock2D: pooling in front of to_in").  in_norm is affine per (sample, channel), to_in and the reducers' first Linear are
linear without bias and act on channels only, so mean_W(Linear_x(to_in(s u + t))) = (W_x W_toin)(s mean_W(u) + t) exactly;
the engine's pooling kernel computes s mean(u) + t (lns_op_fa_pool) and the reducers carry the composed matrix.

Tolerances.  OP_TOL = 2e-6 relative L2, the project's op-level tolerance: a strictly sequential fp32 sum of these rows and
columns stays below 1.9e-7 against float64, so the float64 reference alone leaves a tenfold margin.  STAGE_TOL
(tests/test_gpu_parity.py) for a whole decode and for every FABlock row of the layer trace against the oracle, which keeps
the reference's order (in_norm, to_in, Linear, mean)."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from helpers import rel_l2  # noqa: E402

pytestmark = pytest.mark.gpu

OP_TOL = 2e-6
STAGE_TOL = 2e-5
POOL_SHAPES = [(2, 32, 8, 8), (2, 64, 16, 16), (2, 64, 15, 30), (3, 32, 7, 15), (2, 64, 48, 96), (2, 64, 64, 64)]

_cases = {}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _pool_inputs(B, C, H, W, offsets, seed):
    r = np.random.default_rng(seed)
    x = r.standard_normal((B, C, H, W)).astype(np.float32)
    if offsets:
        x += r.uniform(-3.0, 3.0, (1, C, 1, 1)).astype(np.float32)
    scale = (r.uniform(0.3, 2.0, (B, C)) * r.choice([-1.0, 1.0], (B, C))).astype(np.float32)
    shift = r.uniform(-1.0, 1.0, (B, C)).astype(np.float32)
    return x, np.stack([scale, shift], axis=-1)            # ss [B][C][2]


def _pool_ref(x, ss):
    """float64: mx [B,H,C] = s mean_W(x) + t, my [B,W,C] = s mean_H(x) + t."""
    x = x.astype(np.float64)
    s = ss[..., 0].astype(np.float64) if ss is not None else np.ones(x.shape[:2])
    t = ss[..., 1].astype(np.float64) if ss is not None else np.zeros(x.shape[:2])
    mx = s[:, :, None] * x.mean(axis=3) + t[:, :, None]    # [B,C,H]
    my = s[:, :, None] * x.mean(axis=2) + t[:, :, None]    # [B,C,W]
    return mx.transpose(0, 2, 1), my.transpose(0, 2, 1)


def _pool_gpu(x, ss, pad=0):
    """lns_op_fa_pool on torch's current stream; pad > 0: samples `pad` floats further apart than C*H*W."""
    from lns_amd import _lib
    L = _lib.lib()
    B, C, H, W = x.shape
    per = C * H * W
    buf = torch.full((B, per + pad), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :per] = torch.from_numpy(x.reshape(B, per)).cuda()
    ssd = torch.from_numpy(np.ascontiguousarray(ss)).cuda() if ss is not None else None
    mx = torch.full((B, H, C), float("nan"), dtype=torch.float32, device="cuda")
    my = torch.full((B, W, C), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    rc = L.lns_op_fa_pool(buf.data_ptr(), per + pad, ssd.data_ptr() if ssd is not None else None, B, C, H, W,
                          mx.data_ptr(), my.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, "lns_op_fa_pool rc=%d" % rc
    torch.cuda.synchronize()
    return mx.cpu().numpy(), my.cpu().numpy()


@pytest.mark.parametrize("shape", POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pool_op_matches_float64(shape):
    """Every shape with and without a (scale, shift) table, on zero-mean data and on data with per-channel offsets."""
    _need_gpu()
    for offsets in (False, True):
        x, ss = _pool_inputs(*shape, offsets=offsets, seed=3 + offsets)
        for table in (None, ss):
            mx, my = _pool_gpu(x, table)
            rx, ry = _pool_ref(x, table)
            ex, ey = rel_l2(mx, rx), rel_l2(my, ry)
            print("fa_pool %s offsets=%d ss=%d: mx %.3e my %.3e" % (shape, offsets, table is not None, ex, ey))
            assert np.isfinite(mx).all() and np.isfinite(my).all()
            assert ex < OP_TOL and ey < OP_TOL, (shape, offsets, table is not None, ex, ey)


def test_pool_op_honours_the_batch_stride():
    _need_gpu()
    x, ss = _pool_inputs(3, 32, 7, 15, offsets=True, seed=5)
    mx, my = _pool_gpu(x, ss, pad=37)
    rx, ry = _pool_ref(x, ss)
    ex, ey = rel_l2(mx, rx), rel_l2(my, ry)
    print("fa_pool (3,32,7,15) x_bs = C*H*W + 37: mx %.3e my %.3e" % (ex, ey))
    assert ex < OP_TOL and ey < OP_TOL, (ex, ey)
    m0x, m0y = _pool_gpu(x, ss)
    assert np.array_equal(mx.view(np.int32), m0x.view(np.int32)) and np.array_equal(my.view(np.int32), m0y.view(np.int32))
    from lns_amd import _lib
    p = ctypes.c_void_p(torch.zeros(4, device="cuda").data_ptr())
    assert _lib.lib().lns_op_fa_pool(p, 7, None, 1, 2, 2, 2, p, p, None) == _lib.LNS_EINVAL      # stride below C*H*W


def test_pool_op_is_bit_invariant_to_the_batch():
    """The (2,64,64,64) result equals, bit for bit, samples 0 - 1 of the same call at B = 3."""
    _need_gpu()
    x3, ss3 = _pool_inputs(3, 64, 64, 64, offsets=True, seed=9)
    mx3, my3 = _pool_gpu(x3, ss3)
    mx2, my2 = _pool_gpu(x3[:2], ss3[:2])
    assert np.array_equal(mx2.view(np.int32), mx3[:2].view(np.int32))
    assert np.array_equal(my2.view(np.int32), my3[:2].view(np.int32))


def _fa_layer_names(model):
    return sorted(k[: -len(".in_norm.weight")] for k in model.state_dict() if k.endswith(".in_norm.weight"))


def test_ns2d_64_fablock_rows_and_decode_match_oracle():
    """ns2d_64: the 16 x 16 block runs in_proj and the sandwich as separate kernels, the 32 x 32 block the fused kernel."""
    _need_gpu()
    import gpu_checks as gc
    from lns_amd import config, dropin, filler
    args = config.preset("ns2d_64")
    x = filler.normal("x", (2, args.in_channels, args.Ly, args.Lx), 7)
    rows = gc.layer_trace_compare(args, 1, x)
    fa = _fa_layer_names(dropin.build_dynamics(args))
    dec = {name: err for stage, name, err in rows if stage == "decode"}
    assert len(fa) == 2 and all(n in dec for n in fa), (fa, sorted(dec))
    for n in fa:
        print("ns2d_64 decode %s vs oracle %.3e" % (n, dec[n]))
    print("ns2d_64 decode OUT y vs oracle %.3e" % dec["OUT y"])
    assert all(dec[n] < STAGE_TOL for n in fa), [(n, dec[n]) for n in fa]
    assert dec["OUT y"] < STAGE_TOL, dec["OUT y"]


def test_cond_ae_mini_decode_matches_oracle():
    """Non-square planes: the FABlock of cond_ae_mini works on 14 x 28."""
    _need_gpu()
    from helpers import case_args, load_golden, manifest
    from lns_amd import filler
    from lns_amd.modules.autoencoder2d_nonsquared import ConditionalSimpleAutoencoder
    import lns_oracle
    meta, _ = load_golden("cond_ae_mini")
    args = case_args(meta)
    sd = filler.synthetic_state_dict({k: tuple(v) for k, v in manifest()["cond_ae_mini"].items()}, meta["weight_seed"])
    model = ConditionalSimpleAutoencoder(args)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    model = model.cuda()
    assert _fa_layer_names(model)
    orc = lns_oracle.OracleCondAutoencoder(args, sd, "")
    x = filler.normal("x", (2, args.in_channels, args.Ly, args.Lx), meta["input_seed"])
    param = filler.uniform01("param", 2, meta["input_seed"]).astype(np.float32)
    z_ref = orc.encode(x, param)
    y_ref = orc.decode(z_ref)
    y = model.decode(torch.from_numpy(np.ascontiguousarray(z_ref, dtype=np.float32)).cuda())
    torch.cuda.synchronize()
    err = rel_l2(y.cpu().numpy(), y_ref)
    print("cond_ae_mini decode B=2 vs oracle %.3e" % err)
    assert err < STAGE_TOL, err


def _ns2d_64():
    if "ns2d_64" not in _cases:
        import gpu_checks as gc
        from lns_amd import config, filler
        args = config.preset("ns2d_64")
        model, orc = gc.build_models(args, 1)
        z_ref = orc.x_to_z(filler.normal("x", (2, args.in_channels, args.Ly, args.Lx), 7))
        _cases["ns2d_64"] = (model, z_ref)
    return _cases["ns2d_64"]


CONV1X1_LAUNCHES = 12


def test_ns2d_64_decode_has_no_to_in_launch():
    """The 1x1 class of one ns2d_64 decode, layer by layer (latent 8 x 8, decoder_channels [128, 128, 64, 64], attention at 16
    and 32; with the full-resolution to_in convolutions it was two higher, 14):

      post_quant_conv -> decoder.model.0 (one composed conv, "fold_linear")                        1
      model.1  ResidualBlock 128 -> 128                                                          0
      model.2  SABlock: qkv, proj_out                                                            2
      model.3, model.4, model.5  ResidualBlock 128 -> 128                                        0
      model.6  UpSampleBlock (3x3)                                                               0
      model.7  ResidualBlock 128 -> 64: channel_up                                               1
      model.8  FABlock2D 16 x 16: in_proj, lrk_x.to_qk, lrk_y.to_qk, to_out.1+3                   4
      model.9  UpSampleBlock (3x3)                                                               0
      model.10 ResidualBlock 64 -> 64                                                            0
      model.11 FABlock2D 32 x 32 (in_proj inside the sandwich): lrk_x.to_qk, lrk_y.to_qk, to_out.1+3   3
      model.12 Upsample, model.13 3x3 -> model.14 1x1 (one composed 3x3 conv)                    0
      model.15 GroupNorm, model.16 Swish, model.17 output projection                             1

    Every FABlock2D launches one pooling kernel, one two-axis reducer and one two-axis low-rank kernel.

    GroupNorm class: 7 launches, one more than with to_in.  The in_norm statistics of the 16 x 16 block come out of the
    preceding 3x3 conv's epilogue as two tile partials; in_proj and to_in each merged them in their own prologue, so no
    finalize kernel ran.  The pooling kernel reads the finished (scale, shift) table, so the planner now emits that
    finalize launch (3 us) behind in_proj.  The 32 x 32 block's input split needed the finished table before, too: no change
    there, nor in the flagship's two blocks, which both take that path."""
    _need_gpu()
    model, z_ref = _ns2d_64()
    zd = torch.from_numpy(z_ref).cuda()
    eng = model._engine(zd)
    eng.decode(zd)
    torch.cuda.synchronize()
    eng.timing_enable(True)
    try:
        eng.decode(zd)
        torch.cuda.synchronize()
        t = {k: v["launches"] for k, v in eng.timing().items()}
    finally:
        eng.timing_enable(False)
    print("ns2d_64 decode launches:", sorted(t.items()))
    c1 = [k for k in t if k.startswith("conv1x1") and "/" not in k]
    assert len(c1) == 1, t
    assert t[c1[0]] == CONV1X1_LAUNCHES, t
    assert t["fa_pool"] == 2 and t["fa_reducer"] == 2 and t["fa_lrk"] == 2, t
    assert t["gn_stats"] == 7, t


def test_reloaded_weights_recompose_the_reducer_matrices():
    """A second state_dict loaded into a model that has already run decodes bit for bit like a fresh model built from it:
    W_x W_toin and W_y W_toin are rebuilt by every weight load (after tests/test_fold_gpu.py's reload test)."""
    _need_gpu()
    import gpu_checks as gc
    from helpers import synthetic_state_dict
    from lns_amd import config, filler
    args = config.preset("ns2d_mini")
    used, orc = gc.build_models(args, 1)
    assert _fa_layer_names(used)
    z_ref = orc.x_to_z(filler.normal("x", (2, args.in_channels, args.Ly, args.Lx), 7))
    zd = torch.from_numpy(z_ref).cuda()
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

"""GPU: the dual-phase form of the upsampling 3x3 conv (csrc/conv3_up2d.inc, op-level variant 21).

One block computes both column phases of a (source tile, row phase): the patch is staged once for the two, a lane stores its
pixel pair with one 8-byte store.  The products enter every accumulator in the per-phase form's order and the prologue /
epilogue arithmetic is the same, so the form must give the per-phase form's (variant 17) BITS: outputs, amax side channel
(gpu_checks.conv_case asserts it exactly), GroupNorm tile partials, the decoder's output.  Accuracy is then the per-phase
form's: KERNEL_TOL against the oracle and against float64, as tests/test_gpu_parity.py::test_conv_kernel.

Shapes (source H x W, B = 2): 4 x 32 one exact tile; 6 x 40 ragged in both axes; 16 x 16 two tiles, the plain block order;
32 x 32 eight tiles, the XCD-aware order; 8 x 16 with Cin 40 -> Cout 100, a ragged channel stage and a ragged cout tile;
16 x 16 with 128 -> 128, two cout tiles and sixteen stages -- each with zero and circular padding, with and without bias,
behind a (scale, shift) + Swish prologue, with a GELU epilogue, with a residual and with everything at once; plus
gpu_checks.UP2_CASES and UP2Q_CASES.  The 6 x 40 source gets 2 x 64 tiles, whose 4 x 66 patch is more than one unit per
thread: the per-layer rule refuses it (12 of the 84 listed cases; ragged tiles in both axes run at 10 x 20, 7 x 15, 21 x 13)."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import rel_l2

pytestmark = pytest.mark.gpu

KERNEL_TOL = 2e-6           # tests/test_gpu_parity.py
STAGE_TOL = 2e-5

SHAPES = [dict(H=4, W=32, Cin=64, Cout=64), dict(H=6, W=40, Cin=64, Cout=64), dict(H=16, W=16, Cin=64, Cout=64),
          dict(H=32, W=32, Cin=64, Cout=64), dict(H=8, W=16, Cin=40, Cout=100), dict(H=16, W=16, Cin=128, Cout=128)]
FEATURES = [dict(), dict(bias=False), dict(ss=True, act_in=1), dict(act_out=2), dict(res=True),
            dict(ss=True, act_in=1, act_out=2, res=True, badd=True)]

_done = {}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _cases():
    import gpu_checks as gc
    cases, seen = [], set()
    for c in list(gc.UP2_CASES) + list(gc.UP2Q_CASES):
        if repr(sorted(c.items())) not in seen:
            seen.add(repr(sorted(c.items())))
            cases.append(dict(c))
    for s in SHAPES:
        for mode in ((0, 0), (1, 1)):
            for f in FEATURES:
                cases.append(dict(B=2, up=(2 * s["H"], 2 * s["W"]), mode=mode, **s, **f))
    return cases


def _results():
    """Every case once: (case, y17, y21, err21 vs oracle, err21 vs float64), or (case, None, ...) where the rule refuses it."""
    if "rows" not in _done:
        import gpu_checks as gc
        rows = []
        for i, kw in enumerate(_cases()):
            try:
                e21, _, y21 = gc.conv_case(k=3, variant=21, seed=100 + i, ret_y=True, **kw)
            except AssertionError as ex:
                if "rc=-1" in str(ex):               # the per-layer rule refuses the shape: the planner keeps the per-phase form
                    rows.append((kw, None, None, None, None))
                    continue
                raise
            y17 = gc.conv_case(k=3, variant=17, seed=100 + i, ret_y=True, **kw)[2]
            e64 = gc.conv_case(k=3, variant=21, seed=100 + i, fp64=True, **kw)[2]
            rows.append((kw, y17, y21, e21, e64))
        _done["rows"] = rows
    return _done["rows"]


def _ran(rows):
    ran = [r for r in rows if r[1] is not None]
    n, skipped = len(rows), len(rows) - len(ran)
    assert len(ran) >= 10 and 3 * skipped <= n, "%d of %d listed cases ran, %d refused by the fit rule" % (len(ran), n, skipped)
    return ran


def test_same_bits_as_the_per_phase_form():
    _need_gpu()
    rows = _results()
    ran = _ran(rows)
    print("up2_dual: %d of %d listed cases ran, %d refused by the fit rule" % (len(ran), len(rows), len(rows) - len(ran)))
    for r in rows:
        if r[1] is None:
            print("  refused:", r[0])
    for kw, y17, y21, _, _ in ran:
        assert y17.shape == y21.shape and np.array_equal(y17.view(np.int32), y21.view(np.int32)), kw


def test_accuracy_against_oracle_and_float64():
    _need_gpu()
    worst = (0.0, 0.0)
    for kw, _, _, err, e64 in _ran(_results()):
        worst = (max(worst[0], err), max(worst[1], e64))
        assert err < KERNEL_TOL and e64 < KERNEL_TOL, (kw, err, e64)
    print("up2_dual worst rel-L2: vs oracle %.3e, vs float64 %.3e (bound %.0e)" % (worst[0], worst[1], KERNEL_TOL))


def _conv(x, w, bias, ss, res, mode, variant):
    """lns_op_conv2d of the 2x-upsampled x ([B, Cin, H, W]) with a (scale, shift) + Swish prologue and a residual."""
    from lns_amd import _lib
    L = _lib.lib()
    B, Cin, H, W = x.shape
    Cout = w.shape[0]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    hp = lambda a: np.ascontiguousarray(a, dtype=np.float32).ctypes.data_as(ctypes.c_void_p)
    xd, ssd, resd = dev(x), dev(ss), dev(res)
    y = torch.full((B, Cout, 2 * H, 2 * W), float("nan"), dtype=torch.float32, device="cuda")
    amax = torch.zeros((B, 16), dtype=torch.int32, device="cuda")
    wh, bh = np.ascontiguousarray(w, dtype=np.float32), np.ascontiguousarray(bias, dtype=np.float32)
    rc = L.lns_op_conv2d(xd.data_ptr(), B, Cin, H, W, 2 * H, 2 * W, hp(wh), hp(bh), Cout, 3, 1, 1, 1, 1, 1, 1, mode[0], mode[1],
                         ssd.data_ptr(), 1, 0, resd.data_ptr(), None, y.data_ptr(), variant,
                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), amax.data_ptr())
    assert rc == 0, "lns_op_conv2d rc=%d" % rc
    torch.cuda.synchronize()
    out = y.cpu().numpy()
    assert np.isfinite(out).all()
    return out


@pytest.mark.parametrize("shape", [(64, 64, 10, 20), (40, 100, 16, 16)], ids=["ragged_tiles", "ragged_channels"])
def test_batch_invariance(shape):
    """Samples 0 - 1 of a B = 3 call equal the B = 2 call bit for bit (samples of different magnitudes: the activation scale
    is per sample)."""
    _need_gpu()
    Cin, Cout, H, W = shape
    r = np.random.default_rng(31)
    x = (r.standard_normal((3, Cin, H, W)) * np.array([1.0, 30.0, 1e-3]).reshape(3, 1, 1, 1)).astype(np.float32)
    w = (r.standard_normal((Cout, Cin, 3, 3)) / np.sqrt(9 * Cin)).astype(np.float32)
    bias = (0.1 * r.standard_normal(Cout)).astype(np.float32)
    ss = np.stack([1.0 + 0.2 * r.standard_normal((3, Cin)), 0.1 * r.standard_normal((3, Cin))], -1).astype(np.float32)
    res = r.standard_normal((3, Cout, 2 * H, 2 * W)).astype(np.float32)
    for mode in ((0, 0), (1, 1)):
        y3 = _conv(x, w, bias, ss, res, mode, 21)
        y2 = _conv(x[:2], w, bias, ss[:2], res[:2], mode, 21)
        assert np.array_equal(y3[:2].view(np.int32), y2.view(np.int32)), (shape, mode)
        assert np.array_equal(y3.view(np.int32), _conv(x, w, bias, ss, res, mode, 17).view(np.int32)), (shape, mode)


def _partials(variant, B, Cin, Cout, H, W, mode, res, seed):
    """lns_op_conv_gn without a consumer: (y, tile partials [B][tiles][Cout][2] as stored, geometry) of the upsampling producer,
    or None where the planner's rule attaches no tile statistics to it."""
    from lns_amd import _lib
    L = _lib.lib()
    r = np.random.default_rng(seed)
    x = r.standard_normal((B, Cin, H, W)).astype(np.float32)
    w = np.ascontiguousarray((r.standard_normal((Cout, Cin, 3, 3)) / np.sqrt(9 * Cin)).astype(np.float32))
    bias = np.ascontiguousarray((0.1 * r.standard_normal(Cout)).astype(np.float32))
    resd = torch.from_numpy(r.standard_normal((B, Cout, 2 * H, 2 * W)).astype(np.float32)).cuda() if res else None
    xd = torch.from_numpy(x).cuda()
    ntile = 4 * ((H * W + 127) // 128)
    y = torch.full((B, Cout, 2 * H, 2 * W), float("nan"), dtype=torch.float32, device="cuda")
    part = torch.full((B * ntile * Cout * 2,), float("nan"), dtype=torch.float32, device="cuda")
    ss = torch.full((B, Cout, 2), float("nan"), dtype=torch.float32, device="cuda")
    geom = (ctypes.c_int * 8)(*([-7] * 8))
    a = _lib.LnsConvGnArgs()
    a.x, a.B, a.Cin, a.Hin, a.Win, a.Hv, a.Wv = xd.data_ptr(), B, Cin, H, W, 2 * H, 2 * W
    a.w_host, a.bias_host = w.ctypes.data_as(ctypes.c_void_p), bias.ctypes.data_as(ctypes.c_void_p)
    a.Cout, a.ksize, a.stride, a.dilation = Cout, 3, 1, 1
    a.pad_t = a.pad_b = a.pad_l = a.pad_r = 1
    a.mode_y, a.mode_x = mode
    a.ss, a.act_in, a.act_out, a.residual, a.badd = None, 0, 0, resd.data_ptr() if res else None, None
    a.y, a.tile_variant = y.data_ptr(), variant
    a.part_out, a.part_in, a.geom = part.data_ptr(), None, ctypes.cast(geom, ctypes.c_void_p)
    a.groups, a.eps, a.gamma_host, a.beta_host, a.premul = 4, 1e-5, None, None, None
    a.ss_out = ss.data_ptr()
    rc = L.lns_op_conv_gn(ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    if rc != 0:
        return None
    return y.cpu().numpy(), part.cpu().numpy(), ss.cpu().numpy(), list(geom)


def test_tile_partials_same_bits():
    """The block writes the two slots the two per-phase blocks write, each from that phase's values in the per-phase order:
    stored partials, the finalized (scale, shift) table and the output are equal bit for bit."""
    _need_gpu()
    ran = 0
    for i, (Cin, Cout, H, W) in enumerate([(64, 64, 4, 32), (64, 64, 16, 16), (64, 64, 32, 32), (40, 100, 8, 16), (128, 128, 16, 16),
                                           (64, 64, 8, 64)]):
        for mode in ((0, 0), (1, 1)):
            for res in (False, True):
                p17 = _partials(17, 2, Cin, Cout, H, W, mode, res, 50 + i)
                p21 = _partials(21, 2, Cin, Cout, H, W, mode, res, 50 + i)
                assert (p17 is None) == (p21 is None), (Cin, Cout, H, W, mode, res)
                if p17 is None:
                    continue
                assert p17[3] == p21[3], (p17[3], p21[3])
                used = p17[3][7] * 2 * Cout * 2                     # partials per sample x samples x (mean, M2)
                assert np.isfinite(p17[1][:used]).all() and np.isfinite(p17[2]).all()
                for k in range(3):
                    assert np.array_equal(p17[k].view(np.int32), p21[k].view(np.int32)), (Cin, Cout, H, W, mode, res, k)
                ran += 1
    assert ran >= 8, "%d producer cases carried tile partials" % ran


@pytest.mark.parametrize("preset", ["ns2d_64", "ns2d_mini"])
def test_in_the_decoder(preset):
    """One engine, up2_dual = 1 and = 0: the same bits, both inside STAGE_TOL of the oracle, the same launches per class."""
    _need_gpu()
    import gpu_checks as gc
    from lns_amd import config, filler
    args = config.preset(preset)
    model, orc = gc.build_models(args, 1)
    z_ref = orc.x_to_z(filler.normal("x", (2, args.in_channels, args.Ly, args.Lx), 7))
    y_ref = orc.z_to_x(z_ref)
    zd = torch.from_numpy(z_ref).cuda()
    eng = model._engine(zd)
    ys, launches = {}, {}
    for arm in (1, 0):
        eng.set_option("up2_dual", arm)
        eng.decode(zd)
        torch.cuda.synchronize()
        eng.timing_enable(True)
        try:
            ys[arm] = eng.decode(zd).clone()
            torch.cuda.synchronize()
            launches[arm] = {k: v["launches"] for k, v in eng.timing().items()}
        finally:
            eng.timing_enable(False)
    eng.set_option("up2_dual", 1)
    assert torch.equal(ys[1].view(torch.int32), ys[0].view(torch.int32))
    for arm in (1, 0):
        err = rel_l2(ys[arm].cpu().numpy(), y_ref)
        print("%s decode B=2 up2_dual=%d vs oracle %.3e" % (preset, arm, err))
        assert err < STAGE_TOL, (arm, err)
    print("%s decode launches per class:" % preset, sorted(launches[1].items()))
    assert launches[1] == launches[0], (launches[1], launches[0])

"""GPU: GroupNorm from the tile statistics a convolution leaves in its epilogue, at op level (lns_op_conv_gn): the per-tile
(mean, M2) partials, their merge by the finalize kernels into a (scale, shift) table, and their merge in the prologue of the
consuming convolution (the fold), against float64 on the inputs a randomly initialised network never produces.

Grid, inputs, float64 statements and the derivation of every bound: tests/conv_gn_reference.py.  The reference side of every
comparison is computed from the GPU's own stored y.  Tolerances: the partials' bounds are derived there from the epilogue's
summation tree; the table and the fold are held to KERNEL_TOL per sample, an ill-conditioned sample (big_mean) to
max(KERNEL_TOL, 3 x own); the constant channels of a const_group sample have their own few-ulp assertion.  Every test prints
error, bound and own: those lines are the record of the measured values."""
import ctypes

import numpy as np
import pytest
import torch

import conv_gn_reference as cr

pytestmark = pytest.mark.gpu

NAN = float("nan")
PART_TILES = 64            # room of the partials buffer, in tiles per sample (the grid's largest tiling has 14)
_worst = {"mean": 0.0, "M2": 0.0, "table": 0.0, "fold": 0.0}


def _L():
    from lns_amd import _lib
    assert torch.cuda.is_available(), "GPU test selected but no GPU is visible"
    L = _lib.lib()
    assert L.lns_build_has(b"op_conv_gn") == 1
    return L


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _hp(a):
    return np.ascontiguousarray(a, dtype=np.float32).ctypes.data_as(ctypes.c_void_p) if a is not None else None


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _args(case, inp, samples=None, consumer=None, part_in=None, want_table=True, **over):
    """(LnsConvGnArgs, outputs dict, keep-alive list) for the case's producer on samples `samples` (default: all)."""
    import gpu_checks as gc
    from lns_amd import _lib
    P = cr.PRODUCERS[case["prod"]]
    sl = slice(None) if samples is None else samples
    x = inp["x"][sl]
    B, Cin, Hs, Ws = x.shape
    C, H, W = case["Cout"], case["H"], case["W"]
    oct8 = inp["oct"]
    res = inp["res"][sl] if inp["res"] is not None else None
    keep = [_dev(x), _dev(gc.to_oct8(res) if oct8 else res) if res is not None else None,
            _dev(inp["badd"][sl]) if inp["badd"] is not None else None, _dev(inp["premul"][sl]) if inp["premul"] is not None else None,
            _hp(inp["w"]), _hp(inp["bias"]), _hp(inp["gamma"]), _hp(inp["beta"]), inp]
    out = dict(y=torch.full((B, C, H, W), NAN, dtype=torch.float32, device="cuda"),
               part=torch.full((B * PART_TILES * C * 2,), NAN, dtype=torch.float32, device="cuda"),
               ss=torch.full((B, C, 2), NAN, dtype=torch.float32, device="cuda") if want_table else None,
               geom=(ctypes.c_int * 8)(*([-7] * 8)), y2=None)
    a = _lib.LnsConvGnArgs()
    a.x, a.B, a.Cin, a.Hin, a.Win = keep[0].data_ptr(), B, Cin, Hs, Ws
    a.Hv, a.Wv = (H, W) if P["up"] else (Hs, Ws)
    a.w_host, a.bias_host, a.Cout, a.ksize, a.stride, a.dilation = keep[4], keep[5], C, P["k"], 1, 1
    a.pad_t, a.pad_b, a.pad_l, a.pad_r = inp["pad"]
    a.mode_y, a.mode_x = inp["mode"]
    a.ss, a.act_in, a.act_out, a.residual, a.badd = None, 0, inp["act_out"], _ptr(keep[1]), _ptr(keep[2])
    a.y, a.tile_variant = out["y"].data_ptr(), P["variant"] | (0x200 if oct8 else 0)
    a.part_out, a.part_in, a.geom = out["part"].data_ptr(), _ptr(part_in), ctypes.cast(out["geom"], ctypes.c_void_p)
    a.groups, a.eps, a.gamma_host, a.beta_host, a.premul = case["groups"], cr.eps_of(case), keep[6], keep[7], _ptr(keep[3])
    a.ss_out = _ptr(out["ss"])
    if consumer is not None:
        variant2, ksize2, act_in2 = consumer
        w2, b2 = cr.consumer_weights(case, ksize2)
        keep += [_hp(w2), _hp(b2), w2, b2]
        out["y2"] = torch.full((B, w2.shape[0], H, W), NAN, dtype=torch.float32, device="cuda")
        a.w2_host, a.bias2_host, a.Cout2, a.ksize2, a.act_in2 = keep[-4], keep[-3], w2.shape[0], ksize2, act_in2
        a.variant2, a.y2 = variant2 | (0x100 if oct8 else 0), out["y2"].data_ptr()
    for k, v in over.items():
        setattr(a, k, v)
    return a, out, keep


def _call(L, a):
    rc = L.lns_op_conv_gn(ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


def _y_host(case, inp, out):
    import gpu_checks as gc
    y = out["y"].cpu().numpy()
    if inp["oct"]:
        B, C, H, W = y.shape
        y = gc.from_oct8(y.reshape(B, C // 8, -1, 8), C, H, W)
    return y


def _run(case, inp=None, **kw):
    L = _L()
    inp = inp or cr.case_inputs(case)
    a, out, keep = _args(case, inp, **kw)
    rc = _call(L, a)
    assert rc == 0, (case["name"], rc, L.lns_create_error().decode())
    y = _y_host(case, inp, out)
    assert np.isfinite(y).all(), "non-finite / unwritten producer outputs"
    return inp, out, y


@pytest.mark.parametrize("name", [c["name"] for c in cr.GRID])
def test_partials_and_table(name):
    """The producer's partials against float64 over each tile's valid pixels, then the finalize kernel's table: y * scale +
    shift against the float64 normalisation per sample, the constant channels to a few ulps, gamma = 0 channels exactly."""
    case = cr.BY_NAME[name]
    inp, out, y = _run(case)
    geom = tuple(out["geom"])
    mode, fold, tiles = cr.expected_rule(case)
    assert geom[:5] == cr.expected_geom(case)[:5] and geom[5:] == (mode, int(fold), tiles), (geom, cr.expected_geom(case), mode, fold)
    part = out["part"].cpu().numpy()
    used = case["B"] * tiles * case["Cout"] * 2               # [B][tiles][Cout][2] at the head of a larger NaN-filled buffer
    assert np.isnan(part[used:]).all(), "partials written past the tile count"
    part = part[:used].reshape(case["B"], tiles, case["Cout"], 2).astype(np.float64)
    assert np.isfinite(part).all(), "non-finite / unwritten partials"
    px = cr.tile_pixels(geom, case["H"], case["W"])
    mean, m2, n = cr.partials64(y, px)
    tb, qb, qb0 = cr.partial_bounds(y, px)
    dm, dq = np.abs(part[..., 0] - mean), np.abs(part[..., 1] - m2)

    def ratio(d, bound):                                    # (a zero bound: an exactly zero expectation)
        return float(np.where(bound > 0, d / np.maximum(bound, 1e-300), np.where(d > 0, np.inf, 0.0)).max())
    rm, rq = ratio(dm, tb), ratio(dq, qb)
    _worst["mean"], _worst["M2"] = max(_worst["mean"], rm), max(_worst["M2"], rq)
    print("conv_gn partials %s mode %d tiles %d fold %d: mean err/bound %.3f  M2 err/bound %.3f (%.3f of the bound without its "
          "linear term)" % (name, mode, tiles, fold, rm, rq, ratio(dq, qb0)))
    assert (dm <= tb).all() and (dq <= qb).all(), (name, rm, rq)
    ss = out["ss"].cpu().numpy()
    assert np.isfinite(ss).all(), "non-finite / unwritten table entries"
    scale, shift = ss[..., 0], ss[..., 1]
    for b, err, own, bound in cr.table_errors(case, y, scale, shift, inp):
        _worst["table"] = max(_worst["table"], err / bound)
        print("conv_gn table %s sample %d (%s): err %.3e bound %.3e own %.3e" % (name, b, cr.sample_kind(case, b), err, bound, own))
        assert err <= bound, (name, b, err, bound, own)
    for b, err, bound, ok in cr.const_check(case, y, scale, shift, inp):
        print("conv_gn const %s sample %d: |3.25 scale + shift - beta| %.3e bound %.3e" % (name, b, err, bound))
        assert ok, (name, b, err, bound)
    if case["kind"] == "gamma_zero":
        got = y[:, ::3] * scale[:, ::3, None, None] + shift[:, ::3, None, None]           # float32 throughout
        assert got.dtype == np.float32 and np.array_equal(got, np.broadcast_to(inp["beta"][None, ::3, None, None], got.shape))


# every foldable case with every consumer (an OCT8 producer: the 3x3 consumers, the 1x1 kernel reads planar tensors)
FOLD = [(c["name"], cons) for c in cr.GRID if cr.expected_rule(c)[1] for cons in cr.CONSUMERS
        if not (c["feature"] == "oct" and cons[1] == 1)]


@pytest.mark.parametrize("name,consumer", FOLD, ids=["%s-v%d" % (n, c[0]) for n, c in FOLD])
def test_fold(name, consumer):
    """The merge in the consumer's prologue: y2 against float64 normalisation + activation + convolution per sample; two calls
    give the same bits; the last sample gives the same bits alone as inside the batch."""
    case = cr.BY_NAME[name]
    inp, out, y = _run(case, consumer=consumer, want_table=False)
    y2 = out["y2"].cpu().numpy()
    assert np.isfinite(y2).all(), "non-finite / unwritten consumer outputs"
    w2, b2 = cr.consumer_weights(case, consumer[1])
    ref, bounds, own = cr.fold_bounds(case, y, inp, w2, b2, consumer[1], consumer[2])
    for b in range(case["B"]):
        err = cr.rel(y2[b], ref[b])
        _worst["fold"] = max(_worst["fold"], err / bounds[b])
        print("conv_gn fold %s v%d sample %d (%s): err %.3e bound %.3e own %.3e" % (name, consumer[0], b, cr.sample_kind(case, b), err, bounds[b], own[b]))
        assert err <= bounds[b], (name, consumer, b, err, bounds[b], own[b])
    _, again, _ = _run(case, inp, consumer=consumer, want_table=False)
    assert torch.equal(again["y"], out["y"]) and torch.equal(again["y2"], out["y2"]), "two calls differ"
    b = case["B"] - 1
    _, alone, _ = _run(case, inp, samples=slice(b, b + 1), consumer=consumer, want_table=False)
    assert torch.equal(alone["y"][0], out["y"][b]) and torch.equal(alone["y2"][0], out["y2"][b]), "a sample differs alone"


CRAFTED = ["c3-32x32-C64g32-random", "c1-14x30-C128g1-random", "c3-7x15-C64g1-random-premul", "c3-16x16-C128g32-random",
           "c3-14x30-C64g32-random-premul"]


@pytest.mark.parametrize("name", CRAFTED)
def test_crafted_partials(name):
    """Partials handed in by the caller instead of the producer's: tile means 30 within-tile spreads apart, M2 over four
    decades with exact zeros -- (mean, M2) sets no tensor of the grid produces.  The table against merge64 of the same numbers
    (scale per sample in rel-L2; shift against the size of its two terms), the fold against float64 with that table."""
    case = cr.BY_NAME[name]
    mode, fold, tiles = cr.expected_rule(case)
    B, C = case["B"], case["Cout"]
    n = np.array([len(p) for p in cr.tile_pixels(cr.expected_geom(case), case["H"], case["W"])], np.float64)
    r = np.random.default_rng(len(name))
    mean = (30.0 * r.standard_normal((B, tiles, 1)) + r.standard_normal((B, tiles, C))).astype(np.float32)
    m2 = (n[None, :, None] * 10.0 ** r.uniform(-2, 2, (B, tiles, C))).astype(np.float32)
    m2[:, :, ::5] = 0.0
    pin = _dev(np.stack([mean, m2], -1))
    consumer = cr.CONSUMERS[0] if fold else None
    inp, out, y = _run(case, part_in=pin, consumer=consumer)
    ss = out["ss"].cpu().numpy().astype(np.float64)
    assert np.isfinite(ss).all()
    s64, t64 = cr.merge64(mean.astype(np.float64), m2.astype(np.float64), n, case["groups"], cr.eps_of(case), inp["gamma"], inp["beta"], inp["premul"])
    size = np.abs(np.asarray(inp["beta"], np.float64))[None] + np.abs(np.asarray(inp["beta"], np.float64)[None] - t64)
    for b in range(B):
        es, et = cr.rel(ss[b, :, 0], s64[b]), float(np.sqrt(((ss[b, :, 1] - t64[b]) ** 2).sum() / (size[b] ** 2).sum()))
        print("conv_gn crafted %s sample %d: scale err %.3e shift err %.3e bound %.1e" % (name, b, es, et, cr.KERNEL_TOL))
        assert es <= cr.KERNEL_TOL and et <= cr.KERNEL_TOL, (name, b, es, et)
    if fold:
        w2, b2 = cr.consumer_weights(case, consumer[1])
        ref = cr.fold64(case, y, inp, w2, b2, consumer[1], consumer[2], norm=cr.apply_table(y, s64, t64))
        y2 = out["y2"].cpu().numpy()
        for b in range(B):
            err = cr.rel(y2[b], ref[b])
            print("conv_gn crafted fold %s sample %d: err %.3e bound %.1e" % (name, b, err, cr.KERNEL_TOL))
            assert np.isfinite(y2[b]).all() and err <= cr.KERNEL_TOL, (name, b, err)


def _refusals():
    c = cr._case
    cons = cr.CONSUMERS[0]
    return [
        ("upsampling producer with ragged tiles", c("up", 14, 30, 64, 32), None, {}),
        ("input-stationary 1x1 producer", c("c1", 16, 16, 128, 32), None, dict(tile_variant=8)),
        ("fp32 producer kernel", c("c3", 16, 16, 64, 32), None, dict(tile_variant=-1)),
        ("one exact tile, below 256 pixels", c("c3", 8, 16, 64, 32), None, {}),
        ("1x1 consumer of an OCT8 producer", c("c3", 16, 16, 64, 32, feature="oct"), (7, 1, 1), {}),
        ("groups do not divide Cout", c("c3", 16, 16, 64, 32), None, dict(groups=3)),
        ("eps = 0", c("c3", 16, 16, 64, 32), None, dict(eps=0.0)),
        ("fold of eight partials", c("c3", 32, 32, 64, 32), cons, {}),
        ("fold of ragged tiles", c("c3", 14, 30, 64, 32), cons, {}),
        ("fold with 25 channels per group", c("c3", 16, 16, 100, 4), cons, {}),
        ("fold with premul and several groups", c("c3", 7, 15, 64, 32, premul=True), cons, {}),
        ("fold into the input-stationary 1x1", c("c1", 16, 16, 64, 32), (8, 1, 0), {}),
        ("fold into the bf16x3 3x3 kernel", c("c3", 16, 16, 64, 32), (6, 3, 0), {}),
        ("fold with a GELU prologue", c("c3", 16, 16, 64, 32), (11, 3, 2), {}),
        ("planar consumer of an OCT8 producer", c("c3", 16, 16, 64, 32, feature="oct"), cons, dict(variant2=11)),
    ]


@pytest.mark.parametrize("why,case,consumer,over", _refusals(), ids=[r[0].replace(" ", "_") for r in _refusals()])
def test_refusals(why, case, consumer, over):
    """A combination no plan holds is LNS_EINVAL with a message, and nothing was launched: every output is still NaN."""
    L = _L()
    a, out, keep = _args(case, cr.case_inputs(case), consumer=consumer, **over)
    assert _call(L, a) == -1, why
    msg = L.lns_create_error().decode()
    print("conv_gn refusal (%s): %s" % (why, msg))
    assert msg.startswith("conv_gn: ")
    for k in ("y", "part", "ss", "y2"):
        assert out[k] is None or bool(torch.isnan(out[k]).all()), (why, k)


# ---- plan wiring under a DC offset ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine,B,h,w", [("E1", 2, 16, 16), ("E5", 2, 7, 15), ("E6", 2, 7, 15)])
def test_plan_wiring_under_dc_offset(engine, B, h, w):
    """Engine.propagate with +3.0 on every convolution bias (activations a trained network has and a random one has not)
    against the float64 reference propagator: E1 exact tiles and the fold, E5 one ragged tile, E6 one ragged tile and premul.
    Bound max(STAGE_TOL, 3 x own), own = the same reference in float32 against float64."""
    import train_reference as tr
    from helpers import synthetic_state_dict
    from lns_amd import dropin, filler
    _L()
    e = tr.ENGINES[engine]
    model = dropin.build_dynamics(tr.engine_args(engine))
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    sd = synthetic_state_dict(shapes, tr.WEIGHT_SEED)
    for k in sd:
        if k.endswith(".bias") and len(shapes.get(k[:-4] + "weight", ())) == 4:
            sd[k] = (sd[k] + np.float32(3.0)).astype(np.float32)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    model = model.cuda()
    z = filler.normal("z_in", (B, e["c"], h, w), tr.INPUT_SEED) * np.float32(tr.Z_SCALE)
    prm = filler.uniform01("param", B, tr.INPUT_SEED).astype(np.float32) if e["family"] == "twophase_cond" else None
    zd = _dev(z)
    got = model._engine(zd).propagate(zd, _dev(prm) if prm is not None else None)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    assert np.isfinite(got).all()

    def ref(dtype):
        P = {k: torch.from_numpy(np.ascontiguousarray(sd[k])).to(dtype) for k in tr.prop_shapes(e["family"], e["c"], e["D"], e["blocks"])}
        prop = tr.Propagator(P, e["family"], e["c"], e["D"], e["blocks"], e["dilation"])
        with torch.no_grad():
            return prop(torch.from_numpy(z).to(dtype), torch.from_numpy(prm).to(dtype) if prm is not None else None).double().numpy()
    r64, r32 = ref(torch.float64), ref(torch.float32)
    for b in range(B):
        own, err = cr.rel(r32[b], r64[b]), cr.rel(got[b], r64[b])
        bound = max(cr.STAGE_TOL, 3.0 * own)
        print("conv_gn plan %s %dx%d sample %d: err %.3e bound %.3e own %.3e" % (engine, h, w, b, err, bound, own))
        assert err <= bound, (engine, b, err, bound, own)


def test_zz_report_worst_ratios():
    """The largest error-to-bound ratios the tests above observed in this session (printed for the record)."""
    print("conv_gn worst error / bound: " + "  ".join("%s %.3f" % kv for kv in _worst.items()))
    assert all(v <= 1.0 for v in _worst.values())

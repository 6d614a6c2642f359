"""GPU: the fused FABlock kernels (csrc/fa_fused.inc: fa_gsplit_kernel<2|4>, fa_fused2_kernel<2>, fa_fused_kernel<2>,
fa_fused_g_kernel<2,2,2 | 2,1,1 | 4,1,1>) at op level through lns_op_fa_fused, against the float64 statement of
tests/fa_fused_reference.py (grid, inputs, `own`, `model` and the bounds are described there).

Parity: every grid case, PER PLANE, in rel-L2 and in max |diff| / max |ref|, bound max(KERNEL_TOL, 3 x own) -- for the RELAXED
families (quiet_channel below 2^-8, plane_spread) max(KERNEL_TOL, 3 x own, 3 x model).  Without InstanceNorm this is a check
of absolute scale.  The output is pre-filled with NaN and followed by a 4 KB guard; the all-zero plane of zero_row is exactly 0
with and without InstanceNorm.  max |G| per sample (amax_out) within one ulp of the statement's, never zero.
Same bits: the three 64 x 64 forms, every admissible gpb and 0, b_rev, strided against contiguous x, ss = NULL against an
explicit (1, 0) table, and every sample of a B = 8 (one head) and a B = 9 (three heads) batch against the same sample run alone
-- both branches of the block-to-sample map.
The plan: one 64 x 64 and one 32 x 32 FABlock of ns2d_128.  The layer trace exposes a FABlock's input and its output after
to_out, neither the (scale, shift) table nor Kx / Ky, so the entry cannot be fed the plan's own operands; instead the block's
traced output is compared with the float64 statement of the whole block at KERNEL_TOL (test_plan_fablock_matches_float64).

Measured on an MI355X, worst error / bound over the planes of a family (rel-L2, rel-max); the bound is KERNEL_TOL wherever
3 x own stays below it, which is nearly everywhere:
    plain 0.14 0.22   heavy_w 0.14 0.21   zero_row 0.14 0.23   heavy_k 0.21 0.42   sample_scales 0.17 0.23   big_shift 0.16 0.28
    eps_regime 0.14 0.21   quiet_channel 2^0 0.13 0.23, 2^-4 0.14 0.25, 2^-8 0.25 0.28, 2^-12 0.34 0.34, 2^-16 0.33 0.33
    plane_spread 0.36 0.45
The quiet planes themselves, device | model rel-L2: 2^0 1.9e-7 | 1.3e-7, 2^-4 2.0e-7 | 1.2e-7, 2^-8 5.0e-7 | 4.9e-7, 2^-12
7.7e-6 | 7.7e-6, 2^-16 1.27e-4 | 1.27e-4: KERNEL_TOL holds down to r = 2^-8 on the device as in the model, and beyond it the
device follows the model to three digits (the 0.33 above is the factor 3 of the bound).  The plan: block output 3.7e-7 (64 x 64)
and 4.4e-7 (32 x 32), its change of the input alone 9.4e-7 / 1.0e-6; the entry on the same operands 0.17 / 0.27 of its bound.
No defect found.  The file: 151 tests, 8 s.
"""
import ctypes

import numpy as np
import pytest
import torch

import fa_fused_reference as fr

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD, GUARD_VALUE = 1024, -7.25           # floats after the output
_worst = {}                                # family -> [rel-L2 ratio, rel-max ratio]
_quiet = {}                                # k -> worst device error of the quiet planes, (rel-L2, rel-max)


def _L():
    from lns_amd import _lib
    assert torch.cuda.is_available(), "GPU test selected but no GPU is visible"
    L = _lib.lib()
    assert L.lns_build_has(b"op_fa_fused") == 1
    return L


def _dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float32)).cuda()       # (a copy: the shared references are read-only)


def launch(case, inp, samples=None, **over):
    """lns_op_fa_fused of the case (optionally of the samples `samples` alone, a slice) -> (out [B, planes, H, W], amax [B]) on the
    host.  over: form, gpb, b_rev, strided, ss ("case" / None / an array)."""
    from lns_amd import _lib
    L = _L()
    sl = slice(None) if samples is None else samples
    x, kx, ky = inp["x"][sl], inp["kx"][sl], inp["ky"][sl]
    B, Cin, H, W = x.shape
    planes, n = case["heads"] * case["dh"], Cin * H * W
    ss = over.get("ss", "case")
    ss = (inp["ss"][sl] if inp["ss"] is not None else None) if isinstance(ss, str) else ss
    strided = over.get("strided", case["strided"])
    x_bs = n + fr.GAP if strided else n
    xb = np.full((B, x_bs), np.nan, np.float32)
    xb[:, :n] = x.reshape(B, n)
    w = np.ascontiguousarray(inp["w"], dtype=np.float32)
    keep = [_dev(xb), _dev(ss) if ss is not None else None, _dev(kx), _dev(ky), w]
    nout = B * planes * H * W
    buf = torch.full((nout + GUARD,), NAN, dtype=torch.float32, device="cuda")
    buf[nout:] = GUARD_VALUE
    amax = torch.full((B,), NAN, dtype=torch.float32, device="cuda")
    a = _lib.LnsFaFusedArgs()
    a.x, a.x_bs, a.ss, a.bound = keep[0].data_ptr(), x_bs, keep[1].data_ptr() if ss is not None else None, float(inp["bound"])
    a.w_host, a.kx, a.ky = w.ctypes.data_as(ctypes.c_void_p), keep[2].data_ptr(), keep[3].data_ptr()
    a.B, a.heads, a.dim_head, a.Cin, a.H, a.W, a.eps, a.instnorm = B, case["heads"], case["dh"], Cin, H, W, fr.EPS, case["instnorm"]
    a.form, a.gpb, a.b_rev = over.get("form", case["form"]), over.get("gpb", case["gpb"]), over.get("b_rev", case["b_rev"])
    a.out, a.amax_out = buf.data_ptr(), amax.data_ptr()
    rc = L.lns_op_fa_fused(ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    if rc == _lib.LNS_EHIP:                 # a HIP error: nothing more is started on this device
        pytest.exit("lns_op_fa_fused: HIP error at %s %s" % (case["name"], over), returncode=3)
    torch.cuda.synchronize()
    assert rc == 0, (case["name"], over, rc, L.lns_create_error().decode())
    host = buf.cpu().numpy()
    assert (host[nout:] == GUARD_VALUE).all(), "the guard after the output was written"
    out = host[:nout].reshape(B, planes, H, W)
    assert np.isfinite(out).all(), "non-finite / unwritten outputs"
    return out, amax.cpu().numpy()


_runs = {}


def _run(name):
    """The grid case's launch, once for the tests that share it."""
    if name not in _runs:
        r = fr.reference(name)
        _runs[name] = launch(r["case"], r["inp"])
    return _runs[name]


_measured = {}


def _measure(name):
    """(per-plane errors, error / bound) of the grid case in both measures, once; feeds the per-family record."""
    if name in _measured:
        return _measured[name]
    r = fr.reference(name)
    case = r["case"]
    out, _ = _run(name)
    err = fr.plane_errors(out, r["ref"])
    ratio = [e / b for e, b in zip(err, r["bounds"])]
    w = _worst.setdefault(case["kind"], [0.0, 0.0])
    for k in range(2):
        w[k] = max(w[k], float(ratio[k].max()))
    at = tuple(int(v) for v in np.unravel_index(np.argmax(ratio[1]), ratio[1].shape))
    print("fa_fused %s: rel-L2 %.2e rel-max %.2e (worst plane of each); err/bound %.3f %.3f at (b, plane) = %s; own %.2e %.2e model "
          "%.2e %.2e" % (name, err[0].max(), err[1].max(), ratio[0].max(), ratio[1].max(), at,
                         r["own"][0].max(), r["own"][1].max(), r["model"][0].max(), r["model"][1].max()))
    if case["kind"].startswith("quiet"):
        q = fr.quiet_planes(case)
        k = int(case["kind"][5:])
        e = (float(err[0][:, q].max()), float(err[1][:, q].max()), float(r["model"][0][:, q].max()), float(r["model"][1][:, q].max()))
        _quiet[k] = tuple(max(a, b) for a, b in zip(_quiet.get(k, (0.0,) * 4), e))
        print("   quiet planes (channel at 2^-%d): device rel-L2 %.2e rel-max %.2e, model %.2e %.2e" % ((k,) + e))
    _measured[name] = (err, ratio, at)
    return _measured[name]


@pytest.mark.parametrize("name", [c["name"] for c in fr.GRID])
def test_parity_per_plane(name):
    r = fr.reference(name)
    case = r["case"]
    err, ratio, at = _measure(name)
    if case["kind"] == "zero_row":
        z = _run(name)[0][:, fr.zero_plane(case)]
        assert not z.any(), "the all-zero plane is not exactly zero (instnorm %d)" % case["instnorm"]
    for k, measure in enumerate(("rel-L2", "rel-max")):
        assert (err[k] <= r["bounds"][k]).all(), (name, measure, float(ratio[k].max()), at)


@pytest.mark.parametrize("name", [c["name"] for c in fr.GRID])
def test_amax_out(name):
    """max |G| of every sample as the pre-pass records it: within one float32 ulp of the statement's, never zero."""
    r = fr.reference(name)
    _, amax = _run(name)
    want = r["inp"]["amax"]
    assert amax.dtype == np.float32 and want.dtype == np.float32 and (amax > 0).all(), amax
    ulps = np.abs(amax.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    assert ulps.max() <= 1, (name, amax, want)


def test_report_worst_ratios():
    """The record of the measured values: worst error / bound per family and measure, and the smallest r of quiet_channel at
    which KERNEL_TOL itself still holds on the device, next to the model's."""
    for c in fr.GRID:
        _measure(c["name"])
    for kind in fr.KINDS:
        print("fa_fused worst error / bound, %-13s: rel-L2 %.3f  rel-max %.3f" % ((kind,) + tuple(_worst[kind])))
        assert max(_worst[kind]) <= 1.0
    for k in fr.QUIET:
        print("fa_fused quiet_channel(2^-%d): device rel-L2 %.2e rel-max %.2e | model %.2e %.2e" % ((k,) + _quiet[k]))
    dev = [k for k in fr.QUIET if max(_quiet[k][:2]) <= fr.KERNEL_TOL]
    mod = [k for k in fr.QUIET if max(_quiet[k][2:]) <= fr.KERNEL_TOL]
    print("fa_fused smallest r with the %.0e floor on the quiet planes: device 2^-%d, model 2^-%d" % (fr.KERNEL_TOL, max(dev), max(mod)))
    assert max(dev) >= 8 and max(mod) >= 8


# ---- same bits -----------------------------------------------------------------------------------------------------------
# one fixed case per kernel; dh = 48 and 64 between them hold every admissible gpb
_BASE = {kern: [fr.make_case(kern, 64, 2, 3, 1, "plain", tag="-bits"), fr.make_case(kern, 48, 1, 2, 1, "heavy_k", instnorm=0, tag="-bits")]
         for kern in fr.KERNELS}
_inputs = {}


def _inp(case):
    if case["name"] not in _inputs:
        _inputs[case["name"]] = fr.case_inputs(case)
    return _inputs[case["name"]]


def _first(case):
    key = ("first", case["name"])
    if key not in _runs:
        _runs[key] = launch(case, _inp(case))
    return _runs[key]


def test_forms_give_the_same_bits():
    """The double-buffered, the single-buffered and the generic 64 x 64 kernel."""
    for case in _BASE["b0"]:
        ref, _ = _first(case)
        for form in (1, 2):
            out, _ = launch(case, _inp(case), form=form)
            assert np.array_equal(out.view(np.int32), ref.view(np.int32)), (case["name"], form)


@pytest.mark.parametrize("kern", list(fr.KERNELS))
def test_scheduling_and_layout_give_the_same_bits(kern):
    """gpb (every divisor of dim_head / 16, and 0), b_rev, strided x, ss = NULL against an explicit (1, 0) table."""
    for case in _BASE[kern]:
        inp = _inp(case)
        ref, am = _first(case)
        same = lambda o: np.array_equal(o[0].view(np.int32), ref.view(np.int32)) and np.array_equal(o[1], am)
        for gpb in [g for g in (0, 2, 3, 4) if g == 0 or (case["dh"] // 16) % g == 0]:
            assert same(launch(case, inp, gpb=gpb)), (case["name"], "gpb", gpb)
            assert same(launch(case, inp, gpb=gpb, b_rev=1)), (case["name"], "gpb", gpb, "b_rev")
        assert same(launch(case, inp, strided=True)), (case["name"], "strided")
    case = fr.make_case(kern, 32, 1, 2, 2, "plain", ss_null=True, tag="-bits")
    inp = _inp(case)
    ident = np.zeros((case["B"], case["Cin"], 2), np.float32)
    ident[..., 0] = 1.0
    a, b = launch(case, inp, ss=None), launch(case, inp, ss=ident)
    assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and np.array_equal(a[1], b[1]), case["name"]


@pytest.mark.parametrize("B,heads", [(8, 1), (9, 3)])
@pytest.mark.parametrize("kern", list(fr.KERNELS))
def test_a_sample_does_not_depend_on_its_batch(kern, B, heads):
    """Each sample of the batch against the same sample run alone (B = 1), for both block-to-sample maps ((B & 7) == 0 or
    not), in either block order."""
    case = fr.make_case(kern, 32, heads, B, 2 if heads == 1 else 1, "sample_scales", tight=True, tag="-bits")
    inp = _inp(case)
    for b_rev in (0, 1):
        full, am = launch(case, inp, b_rev=b_rev)
        for b in range(B):
            one, am1 = launch(case, inp, samples=slice(b, b + 1), b_rev=b_rev)
            assert np.array_equal(one[0].view(np.int32), full[b].view(np.int32)), (case["name"], b_rev, b)
            assert am1[0] == am[b]


# ---- the plan ------------------------------------------------------------------------------------------------------------
_plan = {}


def _plan_trace():
    """ns2d_128, B = 2: the decoder's layer trace, the state dict and the prefixes of its FABlocks, once."""
    if not _plan:
        import gpu_checks as gc
        from lns_amd import config, filler
        args = config.preset("ns2d_128")
        model, _ = gc.build_models(args, 1)
        xd = torch.from_numpy(filler.normal("xfa", (2, args.in_channels, args.Ly, args.Lx), 7)).cuda()
        eng = model._engine(xd)
        z = eng.encode(xd)
        eng.trace_enable(True)
        try:
            eng.decode(z)
            torch.cuda.synchronize()
            _plan["trace"] = eng.trace()
        finally:
            eng.trace_enable(False)
        _plan["sd"] = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
        _plan["heads"] = args.attn_heads
    return _plan


@pytest.mark.parametrize("hw", [64, 32])
def test_plan_fablock_matches_float64(hw):
    """A FABlock of the ns2d_128 decoder as the plan runs it (fa_gsplit + the shipped fused kernel, b_rev = 1, automatic gpb),
    and the entry on the same layer's operands, both against float64.  The trace holds layer outputs only -- the block's input
    (the previous layer's output) and the block's output after to_out and the skip --, not the (scale, shift) table or Kx / Ky,
    so bit equality of entry and plan cannot be asked; instead
      plan   the traced block output against fa_block64 of the traced input, rel-L2 per sample below KERNEL_TOL;
      entry  lns_op_fa_fused on the traced input with fa_block64's table, Kx and Ky rounded to float32, the layer's in_proj
             weight and the planner's bound, per plane against the float64 statement: max(KERNEL_TOL, 3 x own)."""
    from helpers import rel_l2
    P = _plan_trace()
    sd, tr, heads = P["sd"], P["trace"], P["heads"]
    names = [n for n, _ in tr]
    pfx = [n for n, a in tr if n + ".in_proj.weight" in sd and a.shape[2] == hw]
    assert len(pfx) >= 1, names
    pfx = pfx[0]
    i = names.index(pfx)
    x, got = tr[i - 1][1], tr[i][1]
    assert i > 0 and x.shape == got.shape and x.shape[2:] == (hw, hw), (names[i - 1], x.shape, got.shape)
    ref, ops = fr.fa_block64(sd, pfx, x, heads)
    for b in range(x.shape[0]):
        e, ed = rel_l2(got[b], ref[b].astype(np.float32)), rel_l2(got[b] - x[b], (ref[b] - x[b]).astype(np.float32))
        print("fa_fused plan %s (%d x %d, %d channels) sample %d: block output rel-L2 %.2e (its change of the input alone: %.2e)"
              % (pfx, hw, hw, x.shape[1], b, e, ed))
        assert e < fr.KERNEL_TOL, (pfx, b, e)
    B, C, H, W = x.shape
    case = dict(name="plan-" + pfx, kind="plan", B=B, Cin=C, H=H, W=W, heads=heads, dh=ops["w"].shape[0] // heads, form=0, gpb=0, b_rev=1,
                instnorm=1, strided=False)
    ss = ops["ss"].astype(np.float32)
    inp = dict(x=x, ss=ss, scale=ss[..., 0], shift=ss[..., 1], w=ops["w"].astype(np.float32), kx=ops["kx"].astype(np.float32),
               ky=ops["ky"].astype(np.float32))
    inp["amax"] = np.abs(fr.fma32(x, inp["scale"][:, :, None, None], inp["shift"][:, :, None, None])).reshape(B, -1).max(axis=1)
    inp["bound"] = np.float32(np.abs(ops["gamma"]).max() * np.sqrt(C * H * W) + np.abs(ops["beta"]).max())
    out, amax = launch(case, inp)
    st = fr.statement64(case, inp)
    err, own = fr.plane_errors(out, st), fr.plane_errors(fr.statement32(case, inp), st)
    for k, measure in enumerate(("rel-L2", "rel-max")):
        bound = np.maximum(fr.KERNEL_TOL, 3.0 * own[k])
        print("fa_fused entry on %s: %s %.2e, err/bound %.3f (own %.2e)" % (pfx, measure, err[k].max(), (err[k] / bound).max(), own[k].max()))
        assert (err[k] <= bound).all(), (pfx, measure, float((err[k] / bound).max()))
    assert np.abs(amax.view(np.int32).astype(np.int64) - inp["amax"].view(np.int32).astype(np.int64)).max() <= 1

"""GPU: the kernels that build a FABlock's Kx / Ky -- fa_reducer_kernel (scalar form), fa_reducer_mfma_kernel,
fa_reducer2_mfma_kernel, fa_lrk_kernel, fa_lrk2_kernel -- at op level through lns_op_fa_reducer / lns_op_fa_lrk, against the
float64 statements of tests/fa_axis_reference.py (shapes, input kinds and tolerances are described there).

Every output is pre-filled with NaN and followed by 64 canary floats: every element must be written, no canary touched.
Errors are relative L2 per sample, for Kx / Ky per (sample, head), and are printed.

Parity     reducer: the six MFMA shapes and the two scalar-form shapes (C % 32 != 0) one launch per axis, three merged launches,
           on zero-mean rows, rows with a per-channel offset (`offset`), rows whose offset to_in turns into a LayerNorm mean of up
           to three standard deviations (`ln_offset`: the first kind does not reach LayerNorm through a random to_in), and rows
           with one zero (constant) row per sample, whose output must be the reducer of beta.  Low-rank kernel: seven shapes
           and two merged launches, both inv_freq vectors, q scaled by 1e-4 and k by 3e3.  With the rotary table as it was
           before its positions followed torch.linspace's single rounding, nine of these sets exceed their tolerance (4e-6 ..
           8e-6 on the x10 sets at n = 15, 24, 48, 96, 160).
Tolerance  KERNEL_TOL = 2e-6, except the offset and ln_offset reducer sets and every low-rank-kernel set: 4 x the float32
           oracle's own error on the same set, the low-rank kernel's measured on the oracle's own positions
           (profiles/fa_axis_parity.json, tools/fa_axis_parity.py).  Measured on the CPU:
           reducer offset sets: oracle 2.2e-7 .. 3.6e-7 -> tolerance 8.7e-7 .. 1.44e-6;
           reducer ln_offset sets: oracle 4.4e-7 .. 7.2e-7 -> 1.8e-6 .. 2.9e-6;
           lrk, either inv_freq vector: oracle 1.3e-7 .. 2.3e-7 -> 5.1e-7 .. 9.3e-7.
Side channel  amax_x[b] is the bit pattern of max |ux[b]| of the stored output, where a block spans samples (n = 7, 15) and
           where a sample's rows lie in two blocks (n = 33, 96, 24 + 48).
Same bits  the merged launch against one launch per axis; samples 0..1 and 1..2 of a B = 3 call against B = 2 calls on those
           samples, at n = 7 and n = 15 (in the second, a row's column inside its 32-row block changes).
Chain      lns_op_fa_pool -> lns_op_fa_reducer -> lns_op_conv2d (k = 1, automatic variant, no bias) -> lns_op_fa_lrk at
           (2, 64, 24, 48) with weights at the oracle's scale against the float64 chain, per (sample, head): the only check in
           which the to_qk convolution runs on reducer outputs, its activation scale taken from the magnitudes the block has.
Plan       a decoder whose FABlock has 128 channels is refused when the plan is built, by layer name and limit.

Measured on an MI355X, worst set of a family: reducer 2.1e-7 .. 3.6e-7 on the zero-mean, offset and zero-row kinds in
every form (the oracle's own 1.8e-7 .. 3.6e-7), 4.0e-7 .. 7.0e-7 on ln_offset; low-rank kernel 1.2e-7 .. 2.5e-7 with either
inv_freq vector, at most a third of its tolerance (2.5e-7 of 7.5e-7 at n = 7, x10); chain u 3.2e-7, Kx 6.9e-7, Ky 6.3e-7.
The file: 74 tests, 2 s."""
import ctypes

import numpy as np
import pytest
import torch

import fa_axis_reference as fr

pytestmark = pytest.mark.gpu

NAN = float("nan")
CANARY, CANARY_VALUE = 64, -7.25


def _L():
    from lns_amd import _lib
    assert torch.cuda.is_available(), "GPU test selected but no GPU is visible"
    L = _lib.lib()
    assert L.lns_build_has(b"op_fa_axis") == 1
    return L


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float32)).cuda()       # (a copy: the shared references are read-only)


def _hp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def guarded(n):
    buf = torch.full((n + CANARY,), NAN, dtype=torch.float32, device="cuda")
    buf[n:] = CANARY_VALUE
    return buf


def read_guarded(buf, shape, what):
    host = buf.cpu().numpy()
    n = int(np.prod(shape))
    assert (host[n:] == CANARY_VALUE).all(), "%s: a canary behind the output was written" % what
    assert not np.isnan(host[:n]).any(), "%s: unwritten outputs" % what
    return host[:n].reshape(shape)


def _rc(rc, what):
    from lns_amd import _lib
    if rc == _lib.LNS_EHIP:                 # a HIP error: nothing more is started on this device
        pytest.exit("%s: HIP error" % what, returncode=3)
    torch.cuda.synchronize()
    assert rc == 0, (what, rc, _lib.lib().lns_create_error().decode())


# ---- reducer ---------------------------------------------------------------------------------------------------------------
def run_reducer(axes, form, samples=None):
    """axes: one or two reducer sets (fa_axis_reference.reducer_set) of the same (B, C, Hid, Out) -> [(u [B, Out, n], amax [B])].
    samples: a slice of the batch."""
    from lns_amd import _lib
    L = _L()
    sl = slice(None) if samples is None else samples
    a = _lib.LnsFaReducerArgs()
    keep, outs = [], []
    r0 = axes[0]
    B = len(range(r0["B"])[sl])
    a.B, a.C, a.Hid, a.Out, a.form = B, r0["C"], r0["Hid"], r0["Out"], form
    for ax, r in zip("xy", axes):
        m = _dev(r["m"][sl])
        w = [np.ascontiguousarray(r["w"][r["tag"] + k]) for k in (".to_in.weight", ".out_ffn.0.weight", ".out_ffn.0.bias",
                                                                 ".out_ffn.1.weight", ".out_ffn.3.weight", ".out_ffn.3.bias")]
        u, am = guarded(B * r["Out"] * r["n"]), guarded(B)
        keep += [m, w]
        outs.append((u, am, (B, r["Out"], r["n"])))
        setattr(a, "m" + ax, m.data_ptr())
        setattr(a, "n" + ax, r["n"])
        for name, arr in zip(("to_in", "ln_g", "ln_b", "w1", "w2", "b2"), w):
            setattr(a, "%s_%s" % (name, ax), _hp(arr).value)
        setattr(a, "u" + ax, u.data_ptr())
        setattr(a, "amax_" + ax, am.data_ptr())
    what = "lns_op_fa_reducer %s form %d" % ("+".join(r["name"] for r in axes), form)
    _rc(L.lns_op_fa_reducer(ctypes.byref(a), _stream()), what)
    return [(read_guarded(u, shape, what), read_guarded(am, (B,), what + " amax")) for u, am, shape in outs]


def check_reducer(r, u, amax):
    err = fr.rel_l2(u, r["ref"], 1)
    print("fa_reducer %-36s rel-L2 per sample, worst %.2e (tolerance %.2e, oracle %.2e)" % (r["name"], err.max(), r["tol"], r["oracle_err"].max()))
    assert np.isfinite(u).all()
    assert (err <= r["tol"]).all(), (r["name"], err, r["tol"])
    if r["kind"] == "const_row":
        want = fr.reducer_beta_row64(r["w"], r["tag"])
        for b, i in enumerate(fr.const_rows(r["B"], r["n"])):
            e = fr.rel_l2(u[b, :, i][None], want[None], 1)[0]
            assert e <= fr.KERNEL_TOL, (r["name"], "the zero row against the reducer of beta", b, i, e)
    # the side channel: the bit pattern of max |u| of the sample, exactly
    want = np.abs(u).reshape(u.shape[0], -1).max(axis=1)
    assert np.array_equal(amax.view(np.int32), want.view(np.int32)), (r["name"], "amax", amax, want)


@pytest.mark.parametrize("kind", fr.KINDS)
@pytest.mark.parametrize("shape", fr.REDUCER_SHAPES, ids=lambda s: "B%dn%dC%dH%dO%d" % s)
def test_reducer_parity(shape, kind):
    """One launch per axis: the MFMA form, or the scalar form where C % 32 != 0."""
    r = fr.reducer_set(kind, *shape)
    (u, amax), = run_reducer([r], 1)
    check_reducer(r, u, amax)


@pytest.mark.parametrize("kind", fr.KINDS)
@pytest.mark.parametrize("case", fr.REDUCER_MERGED, ids=lambda c: "B%dC%dH%dO%d-n%dx%d" % (c[0] + c[1]))
def test_reducer_merged_parity_and_bits(case, kind):
    """Both axes in one launch: parity and amax of each, and the bits of one launch per axis."""
    (B, C, Hid, Out), (nx, ny) = case
    axes = [fr.reducer_set(kind, B, nx, C, Hid, Out, "x"), fr.reducer_set(kind, B, ny, C, Hid, Out, "y")]
    merged = run_reducer(axes, 0)
    for r, (u, amax) in zip(axes, merged):
        check_reducer(r, u, amax)
    both = run_reducer(axes, 1)
    alone = [run_reducer([r], 1)[0] for r in axes]
    for r, (u, amax), (u1, amax1), (u2, amax2) in zip(axes, merged, both, alone):
        for uu, aa in ((u1, amax1), (u2, amax2)):
            assert np.array_equal(u.view(np.int32), uu.view(np.int32)) and np.array_equal(amax.view(np.int32), aa.view(np.int32)), r["name"]


@pytest.mark.parametrize("n", [7, 15])
def test_reducer_sample_does_not_depend_on_its_batch(n):
    """Samples 0..1 and 1..2 of a B = 3 call against B = 2 calls on those samples: the first pair keeps its rows' places and
    loses the neighbour in its last block, the second moves every row to another column of its block."""
    r = fr.reducer_set("offset", 3, n, 64, 128, 64)
    for form in (0, 1):
        axes = [r, fr.reducer_set("offset", 3, 2 * n + 1, 64, 128, 64, "y")] if form == 0 else [r]
        full = run_reducer(axes, form)
        for sl in (slice(0, 2), slice(1, 3)):
            part = run_reducer(axes, form, samples=sl)
            for rr, (u, amax), (u2, amax2) in zip(axes, full, part):
                assert np.array_equal(u[sl].view(np.int32), u2.view(np.int32)), (rr["name"], form, sl)
                assert np.array_equal(amax[sl].view(np.int32), amax2.view(np.int32)), (rr["name"], form, sl)


# ---- low-rank kernel -------------------------------------------------------------------------------------------------------
def run_lrk(axes, form, samples=None):
    """axes: one or two lrk sets -> [K [B, heads, n, n]]."""
    from lns_amd import _lib
    L = _L()
    sl = slice(None) if samples is None else samples
    a = _lib.LnsFaLrkArgs()
    a.form = form
    keep, outs = [], []
    for ax, r in zip("xy", axes):
        B = len(range(r["B"])[sl])
        qk, invf = _dev(r["qk"][sl]), np.ascontiguousarray(r["invf"])
        k = guarded(B * r["heads"] * r["n"] * r["n"])
        keep += [qk, invf]
        outs.append((k, (B, r["heads"], r["n"], r["n"])))
        setattr(a, "qk_" + ax, qk.data_ptr())
        setattr(a, "inv_freq_" + ax, _hp(invf).value)
        setattr(a, "k" + ax, k.data_ptr())
        setattr(a, "B_" + ax, B)
        setattr(a, "heads_" + ax, r["heads"])
        setattr(a, "DK_" + ax, r["DK"])
        setattr(a, "n" + ax, r["n"])
    what = "lns_op_fa_lrk %s form %d" % ("+".join(r["name"] for r in axes), form)
    _rc(L.lns_op_fa_lrk(ctypes.byref(a), _stream()), what)
    return [read_guarded(k, shape, what) for k, shape in outs]


def check_lrk(r, k):
    err = fr.rel_l2(k, r["ref"], 2)
    print("fa_lrk %-28s rel-L2 per (sample, head), worst %.2e (tolerance %.2e, oracle %.2e)" % (r["name"], err.max(), r["tol"], r["oracle_err"].max()))
    assert np.isfinite(k).all()
    assert (err <= r["tol"]).all(), (r["name"], err, r["tol"])


@pytest.mark.parametrize("freq", fr.FREQS)
@pytest.mark.parametrize("shape", fr.LRK_SHAPES, ids=lambda s: "B%dh%dD%dn%d" % s)
def test_lrk_parity(shape, freq):
    r = fr.lrk_set(freq, *shape)
    k, = run_lrk([r], 1)
    check_lrk(r, k)


@pytest.mark.parametrize("freq", fr.FREQS)
@pytest.mark.parametrize("case", fr.LRK_MERGED, ids=lambda c: "B%dh%dD%d-n%dx%d" % (c[0] + c[1]))
def test_lrk_merged_parity_and_bits(case, freq):
    """Both axes in one launch, the LDS sized by the larger: parity of each, and the bits of one launch per axis."""
    (B, heads, DK), (nx, ny) = case
    axes = [fr.lrk_set(freq, B, heads, DK, nx, "x"), fr.lrk_set(freq, B, heads, DK, ny, "y")]
    merged = run_lrk(axes, 0)
    for r, k in zip(axes, merged):
        check_lrk(r, k)
    for r, k, k1 in zip(axes, merged, run_lrk(axes, 1)):
        assert np.array_equal(k.view(np.int32), k1.view(np.int32)), r["name"]


def test_lrk_sample_does_not_depend_on_its_batch():
    axes = [fr.lrk_set("std", 3, 2, 64, 7, "x"), fr.lrk_set("std", 3, 2, 64, 15, "y")]
    for form in (0, 1):
        full = run_lrk(axes, form)
        for sl in (slice(0, 2), slice(1, 3)):
            for r, k, k2 in zip(axes, full, run_lrk(axes, form, samples=sl)):
                assert np.array_equal(k[sl].view(np.int32), k2.view(np.int32)), (r["name"], form, sl)


# ---- the chain -------------------------------------------------------------------------------------------------------------
def test_chain_pool_reducer_to_qk_lrk():
    """The FABlock's way from its normalised input to Kx / Ky, every step an op-level call on the previous one's device output.
    KERNEL_TOL per sample for the reducer outputs and per (sample, head) for Kx / Ky."""
    from lns_amd import _lib
    L = _L()
    c = fr.chain_set()
    B, C, H, W, Out, heads, DK = (c[k] for k in ("B", "C", "H", "W", "Out", "heads", "DK"))
    x, ss = _dev(c["x"]), _dev(c["ss"])
    mx, my = guarded(B * H * C), guarded(B * W * C)
    _rc(L.lns_op_fa_pool(x.data_ptr(), C * H * W, ss.data_ptr(), B, C, H, W, mx.data_ptr(), my.data_ptr(), _stream()), "lns_op_fa_pool")
    read_guarded(mx, (B, H, C), "pool mx"), read_guarded(my, (B, W, C), "pool my")
    a = _lib.LnsFaReducerArgs()
    a.mx, a.my, a.B, a.nx, a.ny, a.C, a.Hid, a.Out, a.form = mx.data_ptr(), my.data_ptr(), B, H, W, C, 2 * C, Out, 0
    keep = []
    u = {"x": guarded(B * Out * H), "y": guarded(B * Out * W)}
    for ax in "xy":
        for name, key in (("to_in", ".to_in.weight"), ("ln_g", ".out_ffn.0.weight"), ("ln_b", ".out_ffn.0.bias"), ("w1", ".out_ffn.1.weight"),
                          ("w2", ".out_ffn.3.weight"), ("b2", ".out_ffn.3.bias")):
            keep.append(np.ascontiguousarray(c["w"]["chain" + ax + key]))
            setattr(a, "%s_%s" % (name, ax), _hp(keep[-1]).value)
        setattr(a, "u" + ax, u[ax].data_ptr())
    _rc(L.lns_op_fa_reducer(ctypes.byref(a), _stream()), "lns_op_fa_reducer (chain)")
    qk = {}
    for ax, n in (("x", H), ("y", W)):
        got = read_guarded(u[ax], (B, Out, n), "chain u" + ax)
        err = fr.rel_l2(got, c["ref"]["u" + ax], 1)
        print("chain u%s: rel-L2 per sample, worst %.2e; max |u| %.3f" % (ax, err.max(), np.abs(got).max()))
        assert (err <= fr.KERNEL_TOL).all(), (ax, err)
        wqk = np.ascontiguousarray(c["w"]["chain%s.to_qk.weight" % ax])
        M = wqk.shape[0]
        qk[ax] = guarded(B * M * n)
        _rc(L.lns_op_conv2d(u[ax].data_ptr(), B, Out, 1, n, 1, n, _hp(wqk), None, M, 1, 1, 1, 0, 0, 0, 0, 0, 0, None, 0, 0, None, None,
                            qk[ax].data_ptr(), -1, _stream(), None), "lns_op_conv2d (chain to_qk)")
        read_guarded(qk[ax], (B, M, n), "chain qk" + ax)
    invf = np.ascontiguousarray(c["invf"])
    k = {"x": guarded(B * heads * H * H), "y": guarded(B * heads * W * W)}
    b = _lib.LnsFaLrkArgs()
    b.qk_x, b.qk_y, b.form, b.nx, b.ny = qk["x"].data_ptr(), qk["y"].data_ptr(), 0, H, W
    b.B_x = b.B_y = B
    b.heads_x = b.heads_y = heads
    b.DK_x = b.DK_y = DK
    b.inv_freq_x = b.inv_freq_y = _hp(invf).value
    b.kx, b.ky = k["x"].data_ptr(), k["y"].data_ptr()
    _rc(L.lns_op_fa_lrk(ctypes.byref(b), _stream()), "lns_op_fa_lrk (chain)")
    for ax, n in (("x", H), ("y", W)):
        got = read_guarded(k[ax], (B, heads, n, n), "chain k" + ax)
        err = fr.rel_l2(got, c["ref"]["k" + ax], 2)
        print("chain K%s: rel-L2 per (sample, head), worst %.2e" % (ax, err.max()))
        assert (err <= fr.KERNEL_TOL).all(), (ax, err)


# ---- the plan --------------------------------------------------------------------------------------------------------------
def test_plan_refuses_a_128_channel_fablock_by_name():
    """decoder_channels = [128, 128, 128, 64] puts a FABlock of 128 channels (Hid 256, Out 64) at 32 x 32: no reducer form
    fits its LDS, and the plan says so when it is built -- not the first launch, with a bare HIP "invalid value"."""
    import gpu_checks as gc
    from lns_amd import _lib, config, filler
    _L()
    args = config.preset("ns2d_64", decoder_channels=[128, 128, 128, 64])
    model, _ = gc.build_models(args, 1)
    xd = torch.from_numpy(filler.normal("x128", (1, args.in_channels, args.Ly, args.Lx), 7)).cuda()
    with pytest.raises(_lib.LnsError) as ei:        # (lns_prepare builds the decoder's plan with the encoder's)
        eng = model._engine(xd)
        eng.decode(eng.encode(xd))
    msg = str(ei.value)
    print("plan refusal:", msg)
    assert "no PoolingReducer kernel" in msg and "C = 128" in msg and "199680" in msg and "163840" in msg and "decoder" in msg, msg

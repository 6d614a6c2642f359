"""GPU (-m gpu): energy spectra with a basis per axis (include/lns.h "energy spectra", "a basis per axis").

The op (lns_op_energy_spectrum_basis) under the three bases with a DCT axis against the float64 dense-matrix transform of
tests/spectrum_basis_reference.py, per spectrum and bin, under the bound of the DFT spectra
    |E - E64| <= 2e-5 * E64 + 2e-7 * sum(E64)
(tests/test_spectrum_basis_cpu.py shows it admissible for the new bases: 3 x the float32 numpy statement stays below it).
As in tests/test_eval_spectrum_gpu.py, the error row's reference transforms d = P - Q formed in fp32 by the statement's map.

DFT / DFT through the new entry point is lns_op_energy_spectrum bit for bit.  The streaming calls with the option
"spectrum_basis" (the wrappers' basis= / spectrum_basis=) equal the op on the stored rollout BIT FOR BIT, whatever the
scheduling options; a call without the keyword afterwards returns the DFT spectra again (the option was put back)."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import spectrum_basis_reference as br  # noqa: E402
import spectrum_reference as sr  # noqa: E402
import test_eval_gpu as teg  # noqa: E402

pytestmark = pytest.mark.gpu

B, T, KEEP = teg.B, teg.T, teg.KEEP
_same = teg._same
# 33x33: a second row tile and a second column tile of one element; 192x96: six row tiles, the largest LDS image
PLANES = [(1, 7), (2, 2), (3, 5), (16, 16), (32, 32), (33, 33), (24, 40), (61, 121), (96, 192), (192, 96)]
NAME = {br.DFT: "dft", br.DCT: "dct"}


def _names(basis):
    return NAME[basis[0]], NAME[basis[1]]


def _has_basis():
    from lns_amd import _lib
    assert _lib.lib().lns_build_has(b"spectrum_basis") == 1


def _op(y_hat, y=None, basis=(br.DFT, br.DFT), **norm):
    from lns_amd import metrics
    out = metrics.energy_spectrum(torch.from_numpy(y_hat).cuda(), None if y is None else torch.from_numpy(y).cuda(),
                                  basis=_names(basis), **norm)
    torch.cuda.synchronize()
    return out


_CASES = {}


def _cases(H, W):
    """The inputs of a plane, made once and shared (never written to)."""
    if (H, W) not in _CASES:
        _CASES[(H, W)] = br.cases(H, W)
    return _CASES[(H, W)]


@pytest.mark.parametrize("basis", br.NEW, ids=lambda b: br.NAMES[b].replace(",", "-"))
@pytest.mark.parametrize("plane", PLANES, ids=lambda p: "%dx%d" % p)
def test_op_against_float64(plane, basis):
    """Measured worst |E - E64| / bound per plane on MI355X, (dct,dft) / (dft,dct) / (dct,dct), all three spectra and all
    inputs of spectrum_basis_reference.cases:
        1x7     0.039 / 0.045 / 0.045        33x33   0.055 / 0.032 / 0.038
        2x2     0.026 / 0.018 / 0.022        24x40   0.034 / 0.029 / 0.042
        3x5     0.046 / 0.043 / 0.052        61x121  0.065 / 0.043 / 0.044
        16x16   0.050 / 0.036 / 0.031        96x192  0.097 / 0.054 / 0.082
        32x32   0.060 / 0.028 / 0.039        192x96  0.155 / 0.121 / 0.100
    (the largest on the cosine-synthesised steep field under mean / std = 310 / 180).
    Parseval: sum_s E[s] against mean(u^2) in float64, to 1e-5 (measured: 1.1e-6 at most)."""
    teg._need_gpu()
    _has_basis()
    H, W = plane
    S = br.bins(H, W, *basis)
    worst = 0.0
    for name, y_hat, y, norm in _cases(H, W):
        e64 = br.spectra64(y_hat, y, basis, **norm)
        e = _op(y_hat, y, basis, **norm).cpu().numpy()
        assert e.shape == (sr.B, sr.T, sr.C, 3, S) and e.dtype == np.float32
        ratio = br.worst_ratio(e, e64)
        fields = sr._fields(y_hat, y, norm, np.float32)
        ms = np.stack([(u.astype(np.float64) ** 2).mean((-2, -1)) for u in fields], -1)
        parseval = float((np.abs(e.astype(np.float64).sum(-1) - ms) / ms).max())
        print("%s [%s]: worst |E - E64| / bound = %.4f, Parseval %.2e" % (name, br.NAMES[basis], ratio, parseval))
        worst = max(worst, ratio) if ratio == ratio else float("nan")
        assert ratio <= 1.0, (name, ratio)
        assert parseval <= 1e-5, (name, parseval)
        e0 = _op(y_hat, None, basis, **norm).cpu().numpy()              # without the truth: row 0 alone, the same bits
        assert e0.shape == (sr.B, sr.T, sr.C, 1, S)
        assert np.array_equal(e0[..., 0, :].view(np.int32), e[..., 0, :].view(np.int32)), name
    print("%dx%d [%s]: worst ratio ours / bound = %.4f" % (H, W, br.NAMES[basis], worst))


def test_single_mode_and_constant_fields():
    teg._need_gpu()
    _has_basis()
    H, W = 24, 40
    mode = br.wall_mode(H, W, 3, 2)
    u = np.stack([mode, np.full((H, W), 1.75), np.zeros((H, W))])[None, None].astype(np.float32)           # [1, 1, 3, H, W]
    for basis in br.BASES:
        S = br.bins(H, W, *basis)
        e = _op(u, None, basis).cpu().numpy().astype(np.float64)[0, 0, :, 0]
        assert e.shape == (3, S)
        const = np.zeros(S)
        const[0] = 1.75 ** 2                                             # a constant field: bin 0 under every basis
        assert np.all(np.abs(e[1] - const) <= sr.REL * const + sr.ABS * const.sum()), (basis, np.abs(e[1] - const).max())
        assert np.all(e[2] == 0.0)
        if basis == (br.DCT, br.DFT):                                    # half units: 3^2 + (2 * 2)^2 = 5^2
            expect = np.zeros(S)
            expect[5] = 0.25
            assert np.all(np.abs(e[0] - expect) <= sr.REL * expect + sr.ABS * expect.sum()), np.abs(e[0] - expect).max()
        # the error of a forecast against itself is exactly zero, whatever the normalisation
        e3 = _op(u, u, basis, mean=310.0, std=180.0).cpu().numpy()
        assert np.all(e3[..., 2, :] == 0.0) and np.array_equal(e3[..., 0, :], e3[..., 1, :])


@pytest.mark.parametrize("basis", br.NEW, ids=lambda b: br.NAMES[b].replace(",", "-"))
def test_nan_pixel_stays_in_its_plane(basis):
    teg._need_gpu()
    _has_basis()
    name, y_hat, y, norm = _cases(33, 33)[0]
    clean = _op(y_hat, y, basis, **norm).cpu().numpy()
    y_hat = y_hat.copy()
    y_hat[1, 0, 2, 17, 30] = np.nan
    e = _op(y_hat, y, basis, **norm).cpu().numpy()
    bad = np.isnan(e)
    assert bad[1, 0, 2, 0].all() and bad[1, 0, 2, 2].all() and not bad[1, 0, 2, 1].any()      # forecast and error; not the truth
    bad[1, 0, 2] = False
    assert not bad.any()
    keep = np.ones(e.shape, bool)
    keep[1, 0, 2, (0, 2)] = False
    assert np.array_equal(e[keep].view(np.int32), clean[keep].view(np.int32))


@pytest.mark.parametrize("plane", PLANES, ids=lambda p: "%dx%d" % p)
def test_dft_dft_through_the_basis_entry_point_is_the_old_op(plane):
    teg._need_gpu()
    _has_basis()
    from lns_amd import _lib, engine
    L = _lib.lib()
    H, W = plane
    S = sr.bins(H, W)
    assert L.lns_spectrum_bins_basis(H, W, 0, 0) == S
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for name, y_hat, y, norm in _cases(H, W)[1::2]:                     # the harsher normalisation of each kind
        yh, yt = torch.from_numpy(y_hat).cuda(), torch.from_numpy(y).cuda()
        spec = engine.eval_spec(sr.C, **norm)
        old = torch.empty((sr.B, sr.T, sr.C, 3, S), dtype=torch.float32, device="cuda")
        new = torch.full_like(old, float("nan"))
        a = (yh.data_ptr(), yt.data_ptr(), sr.B, sr.T, sr.C, H, W, ctypes.byref(spec))
        assert L.lns_op_energy_spectrum(*a, old.data_ptr(), stream) == 0
        assert L.lns_op_energy_spectrum_basis(*a, new.data_ptr(), stream, 0, 0) == 0
        torch.cuda.synchronize()
        assert _same(old, new), name


# ---- streaming ----------------------------------------------------------------------------------------------------------
def _reference(eng, out, yd, steps, norm, basis):
    idx = list(range(T)) if steps is None else list(steps)
    ref = eng.energy_spectrum(out[:, idx].contiguous(), yd[:, idx].contiguous(), basis=basis, **norm)
    torch.cuda.synchronize()
    return idx, ref


@pytest.mark.parametrize("case,basis", [("ns2d_mini", "dct"), ("ns2d_mini", ("dct", "dft")), ("twophase_cond", "auto")],
                         ids=["ns2d_mini-dct-dct", "ns2d_mini-dct-dft", "twophase_cond-auto"])
def test_streaming_spectra_same_bits_as_the_op_on_the_stored_rollout(case, basis):
    teg._need_gpu()
    _has_basis()
    from lns_amd import metrics
    args, model, eng, xd, yd, pd, norm, denorm, y = teg._setup(case)
    out, f_ref, s_ref = teg._two_call(eng, xd, yd, pd, norm)
    names = eng._basis_names(basis)
    if basis == "auto":
        assert names == ("dct", "dct")                                   # the two-phase tank has walls on all four sides
    S = eng.spectrum_bins(basis=basis)
    assert S == br.bins(args.Ly, args.Lx, *metrics.spectrum_basis(names)) != eng.spectrum_bins()
    old = eng.rollout_eval_spectrum(xd, yd, param=pd, keep_steps=KEEP, spectrum_steps=(0, 3, 4), **norm)
    torch.cuda.synchronize()
    for steps in ((0, 3, 4), None):
        idx, ref = _reference(eng, out, yd, steps, norm, basis)
        for keep in (KEEP, ()):
            r = eng.rollout_eval_spectrum(xd, yd, param=pd, keep_steps=keep, spectrum_steps=steps, basis=basis, **norm)
            torch.cuda.synchronize()
            assert r.spectra.shape == (B, len(idx), args.in_channels, 3, S) and list(r.spectrum_steps) == idx
            assert _same(r.spectra, ref), (case, steps, keep)
            assert _same(r.frame, f_ref) and _same(r.seq, s_ref), (case, steps, keep)
            if keep:
                assert _same(r.frames, out[:, list(keep)].contiguous())
            else:
                assert r.frames is None
            assert eng.options.get("spectrum_basis", 0) == 0
    # the option was put back: a call without the keyword returns the old S and the old bits
    again = eng.rollout_eval_spectrum(xd, yd, param=pd, keep_steps=KEEP, spectrum_steps=(0, 3, 4), **norm)
    torch.cuda.synchronize()
    assert again.spectra.shape[-1] == eng.spectrum_bins() == sr.bins(args.Ly, args.Lx)
    assert _same(again.spectra, old.spectra) and _same(again.frame, old.frame)
    # the spectra are what float64 says of the same stored fields
    idx, ref = _reference(eng, out, yd, None, norm, basis)
    e64 = br.spectra64(out.cpu().numpy(), y, metrics.spectrum_basis(names), **norm)
    ratio = br.worst_ratio(ref.cpu().numpy(), e64)
    print("%s %s: streaming spectra against float64 of the stored rollout, worst ratio to the bound %.4f" % (case, names, ratio))
    assert ratio <= 1.0
    # carried by the stats call and by the maps call, and by the drop-in
    st = eng.rollout_eval_stats(xd, yd, param=pd, keep_steps=KEEP, stats_steps=(1,), spectrum_steps=(0, 3, 4),
                                spectrum_basis=basis, **norm)
    mp = eng.rollout_eval_maps(xd, yd, param=pd, keep_steps=KEEP, spectrum_steps=(0, 3, 4), spectrum_basis=basis, **norm)
    torch.cuda.synchronize()
    for r in (st, mp):
        assert _same(r.spectra, ref[:, [0, 3, 4]].contiguous()) and _same(r.frame, f_ref) and _same(r.seq, s_ref)
        assert _same(r.frames, out[:, list(KEEP)].contiguous())
    extra = (pd,) if pd is not None else ()
    v = model.validate_spectrum(xd, yd, *extra, spectrum_steps=slice(None, None, 2), keep_steps=KEEP, spectrum_basis=basis, **norm)
    torch.cuda.synchronize()
    assert list(v.spectrum_steps) == [0, 2, 4] and _same(v.spectra, ref[:, [0, 2, 4]].contiguous())
    assert _same(v.frame, f_ref) and _same(v.frames, out[:, list(KEEP)].contiguous())


def test_streaming_spectra_do_not_depend_on_scheduling_options():
    teg._need_gpu()
    _has_basis()
    args, model, eng, xd, yd, pd, norm, denorm, y = teg._setup("ns2d_mini")
    out, f_ref, s_ref = teg._two_call(eng, xd, yd, pd, norm)
    steps = (0, 3, 4)
    refs = {b: _reference(eng, out, yd, steps, norm, b)[1] for b in ("dct", ("dct", "dft"))}
    keep_ref = out[:, list(KEEP)].contiguous()
    grid = [(dg, ds, 1) for dg in (1, 2, 3, 0) for ds in (1, 2, 3, 4)] + [(dg, 1, 0) for dg in (1, 2, 3, 0)]
    for dg, ds, ov in grid:
        eng.set_option("decode_group", dg)
        eng.set_option("decode_streams", ds)
        eng.set_option("overlap", ov)
        for b, ref in refs.items():
            r = eng.rollout_eval_spectrum(xd, yd, param=pd, keep_steps=KEEP, spectrum_steps=steps, basis=b, **norm)
            torch.cuda.synchronize()
            assert _same(r.spectra, ref) and _same(r.frame, f_ref) and _same(r.seq, s_ref) and _same(r.frames, keep_ref), (dg, ds, ov, b)


@pytest.mark.parametrize("case,basis", [("ns2d_mini", "dct"), ("twophase_cond", "auto")], ids=["ns2d_mini-dct-dct", "twophase_cond-auto"])
def test_chunked_latent_calls_reproduce_the_one_call_result(case, basis):
    teg._need_gpu()
    _has_basis()
    args, model, eng, xd, yd, pd, norm, denorm, y = teg._setup(case)
    one = eng.rollout_eval_spectrum(xd, yd, param=pd, keep_steps=KEEP, basis=basis, **norm)
    torch.cuda.synchronize()
    z0 = eng.encode(xd) if not eng.cfg.cond_encoder else eng.encode(xd, pd)
    a = eng.rollout_latent_eval_spectrum(z0, yd, steps=3, t0=0, param=pd, keep_steps=(0,), spectrum_steps=(0, 1, 2), basis=basis, **norm)
    b = eng.rollout_latent_eval_spectrum(a.z_last, yd, steps=2, t0=3, param=pd, keep_steps=(0, 1), spectrum_steps=None,
                                         frame=a.frame, seq=a.seq, basis=basis, **norm)
    torch.cuda.synchronize()
    assert _same(torch.cat([a.spectra, b.spectra], 1), one.spectra), case
    assert _same(b.frame, one.frame) and _same(b.seq, one.seq)
    assert _same(torch.cat([a.frames, b.frames], 1), one.frames)
    # the latent forms of the stats and maps calls carry the same spectra
    s = eng.rollout_latent_eval_stats(a.z_last, yd, steps=2, t0=3, param=pd, stats_steps=(0,), spectrum_steps=(1,),
                                      frame=a.frame, seq=a.seq, spectrum_basis=basis, **norm)
    torch.cuda.synchronize()
    assert _same(s.spectra, one.spectra[:, 4:5].contiguous())


def test_workspace_is_the_evaluation_workspace():
    teg._need_gpu()
    _has_basis()
    from lns_amd import _lib, engine
    args, model, eng, xd, yd, pd, norm, denorm, y = teg._setup("ns2d_mini")
    L, h = eng._L, eng._h
    n1 = ctypes.c_size_t(0)
    assert L.lns_rollout_eval_workspace_bytes(h, B, ctypes.byref(n1)) == 0
    assert L.lns_set_option(h, b"spectrum_basis", 3) == 0
    try:
        n2 = ctypes.c_size_t(0)
        assert L.lns_rollout_eval_workspace_bytes(h, B, ctypes.byref(n2)) == 0 and n2.value == n1.value
        C = args.in_channels
        spec = engine.eval_spec(C, **norm)
        S = L.lns_spectrum_bins_basis(args.Ly, args.Lx, 1, 1)
        frame = torch.empty((B, T, C), dtype=torch.float32, device="cuda")
        seq = torch.empty((B, C), dtype=torch.float32, device="cuda")
        spectra = torch.empty((B, T, C, 3, S), dtype=torch.float32, device="cuda")
        ws = torch.empty(n1.value, dtype=torch.uint8, device="cuda")
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        sel = (ctypes.c_int * T)(*range(T))

        def run(nbytes):
            return L.lns_rollout_eval_spectrum(h, xd.data_ptr(), None, yd.data_ptr(), B, T, ctypes.byref(spec), frame.data_ptr(),
                                               seq.data_ptr(), None, 0, None, ws.data_ptr(), nbytes, stream, sel, T, spectra.data_ptr())
        assert run(n1.value - 1) == _lib.LNS_ENOMEM and "workspace" in L.lns_last_error(h).decode()
        assert run(n1.value) == 0
        torch.cuda.synchronize()
    finally:
        assert L.lns_set_option(h, b"spectrum_basis", 0) == 0
    out, f_ref, s_ref = teg._two_call(eng, xd, yd, pd, norm)
    _, ref = _reference(eng, out, yd, None, norm, "dct")
    assert _same(spectra, ref) and _same(frame, f_ref) and _same(seq, s_ref)

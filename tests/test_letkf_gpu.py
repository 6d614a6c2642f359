"""GPU (-m gpu): the localised ensemble transform Kalman filter (lns_op_ensemble_patch_gram, lns_op_letkf_combine,
lns_op_ensemble_transform_local, lns_rollout_latent_ensemble_analysis_local, include/lns.h; Engine.ensemble_patch_gram /
letkf_combine / ensemble_transform_local / rollout_latent_ensemble_analysis_local, enkf.LocalEnsembleFilter,
LatentDynamics.assimilate_ensemble(loc_radius=...)).

The patch sums are held to the project's rule against tests/letkf_reference.py: max(1e-12, 3 x own) in rel-L2 and in max|diff| /
max|ref|, own = the reference's float64 form against its longdouble form on the same inputs.  Combine (the taper included) and the
update are held bit for bit to the order-exact float64 statement.  The engine call is held bit for bit to the ops applied to the
member fields that `rollout_latent` at batch B * M with keep_steps produces, over the scheduling grid of tests/test_etkf_gpu.py,
whose cases, references and helpers this file shares.  RATIOS collects the worst ratio to the bound per case
(tools/letkf_parity.py writes it to profiles/letkf_parity.json)."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import etkf_reference as er  # noqa: E402
import letkf_reference as lr  # noqa: E402
import test_etkf_gpu as eg  # noqa: E402
from ensemble_exceed_reference import SCALAR, per_channel_norm  # noqa: E402

pytestmark = pytest.mark.gpu

B, M, T, RHO = eg.B, eg.M, eg.T, eg.RHO
DSENTINEL = eg.DSENTINEL
RATIOS = {}                                           # case -> worst ratio to the bound (tools/letkf_parity.py)
_same, _stream, _guarded, _guards_intact, _placed = eg._same, eg._stream, eg._guarded, eg._guards_intact, eg._placed


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from lns_amd import _lib
    assert _lib.lib().lns_build_has(b"ensemble_letkf") == 1


# ---- the patch Gram op ---------------------------------------------------------------------------------------------------------
def _patch_gram_op(frames, y, rinv, r_bs, r_ss, grid, norm, off=0):
    """lns_op_ensemble_patch_gram through ctypes: inputs optionally one float off a 16-byte boundary, the output pre-filled with a
    sentinel between guard words that must survive; called twice, the second call must give the first one's bits."""
    from lns_amd import _lib, engine
    L = _lib.lib()
    n, b, m, c, h, w = frames.shape
    E = m * m + m + 3
    spec = engine.eval_spec(c, **norm) if norm else None
    src, obs, rv = _placed(frames, off), _placed(y, off), _placed(rinv, off)
    outs = []
    for _ in range(2):
        buf, view = _guarded(b * n * grid[0] * grid[1] * E)
        rc = L.lns_op_ensemble_patch_gram(src.data_ptr(), obs.data_ptr(), rv.data_ptr(), r_bs, r_ss, n, b, m, c, h, w, grid[0], grid[1],
                                          ctypes.byref(spec) if spec is not None else None, view.data_ptr(), _stream())
        assert rc == 0, (rc, L.lns_create_error())
        torch.cuda.synchronize()
        assert _guards_intact(buf, view.numel()) and not bool((view == DSENTINEL).any())
        outs.append(view)
    assert _same(outs[0], outs[1])
    return outs[0].view(b, n, grid[0] * grid[1], E).cpu().numpy()


PLANE_GRIDS = (((1, 1), (1, 1)), ((1, 7), (1, 3)), ((3, 5), (2, 2)), ((3, 5), (4, 4)), ((17, 16), (4, 4)), ((61, 121), (7, 15)))
# (q, B, n, C): q = 0: shared weights, no norm, aligned; q = 1: per-sample strided weights, scalar norm, inputs one float off a
# 16-byte boundary and NaN / +-inf wherever rinv = 0; q = 2: per-step weights, the per-channel norm
_COMBOS = ((0, 1, 1, 1), (1, 2, 2, 3), (2, 1, 2, 2))


@pytest.mark.parametrize("hw,grid", PLANE_GRIDS, ids=lambda p: "%dx%d" % p)
@pytest.mark.parametrize("m", [2, 3, 7, 33, 64])
def test_patch_gram_op_under_the_rule(m, hw, grid):
    """M x (plane, grid) over the three shapes of _COMBOS, the four input families in turn: every patch's G, g and stat within
    max(1e-12, 3 x own) of the longdouble statement (etkf_reference.gram on the values of one patch at a time) in both
    distances; G symmetric to the bit; the counts exact; an empty patch (3 x 5 on 4 x 4) all zero; the patches add up to the
    global count.  The reference sees the clean inputs, the device NaN / inf at the unobserved values."""
    _need_gpu()
    h, w = hw
    worst = 0.0
    for q, b, n, c in _COMBOS:
        family = er.FAMILIES[(q + m) % 4][0]
        fr, yy = er.family_inputs((n, b, m, c, h, w), 2000 * m + 7 * h + w + q, family)
        per_sample, per_step = q == 1, q == 2
        density = 0.25 if h * w > 1000 else 0.6
        r = er.rinv_map((b, n, c, h, w), 60 + q + m, density=density, per_sample=per_sample, per_step=per_step)
        norm = (None, SCALAR, per_channel_norm(c))[q]
        per = c * h * w
        r_bs, r_ss = (n * per if per_sample else 0), (per if per_step or per_sample else 0)
        full_r = np.broadcast_to(r, (b, n, c, h, w))
        r_dev = np.ascontiguousarray(full_r if per_sample else r).copy()
        fr_dev, yy_dev = fr.copy(), yy.copy()
        if q == 1:
            hole = ~(full_r > 0)
            yy_dev[hole] = np.nan
            holes = np.broadcast_to(hole.transpose(1, 0, 2, 3, 4)[:, :, None], fr.shape)
            fr_dev[holes & (np.arange(m).reshape(1, 1, m, 1, 1, 1) % 2 == 0)] = np.inf
            fr_dev[holes & (np.arange(m).reshape(1, 1, m, 1, 1, 1) % 2 == 1)] = -np.nan
        got = _patch_gram_op(torch.from_numpy(fr_dev).cuda(), torch.from_numpy(yy_dev).cuda(), torch.from_numpy(r_dev).cuda(), r_bs, r_ss,
                             grid, norm, off=q & 1)
        p64, pld = lr.patch_gram(fr, yy, full_r, grid, norm), lr.patch_gram(fr, yy, full_r, grid, norm, dt=er.LD)
        tag = (m, h, w, grid, q, family)
        mm = m * m
        for name, sl in (("G", slice(0, mm)), ("g", slice(mm, mm + m)), ("stat", slice(mm + m, mm + m + 3))):
            ok, ratio, dist, lim = er.held(got[..., sl], p64[..., sl], pld[..., sl])
            worst = max(worst, ratio)
            print("patch gram", tag, name, "%.3g of the bound" % ratio)
            assert ok, tag + (name, dist, lim)
        G = got[..., :mm].reshape(b, n, -1, m, m)
        assert np.array_equal(G, G.transpose(0, 1, 2, 4, 3)), tag
        pidx = lr.patch_index(h, w, grid[0], grid[1])
        counts = np.stack([(full_r > 0)[..., pidx == t].sum(-1).sum(-1) for t in range(grid[0] * grid[1])], -1)   # [b, n, patches]
        assert np.array_equal(got[..., mm + m + 2], counts), tag
        for t in range(grid[0] * grid[1]):
            if not (pidx == t).any():
                assert not got[:, :, t].any(), tag + (t,)
    RATIOS["patch gram M=%d %dx%d on %dx%d" % ((m,) + hw + grid)] = worst


# ---- the combine op ------------------------------------------------------------------------------------------------------------
def _combine_op(part, grid, radius, bc, m):
    from lns_amd import _lib
    L = _lib.lib()
    b, n, hw, E = part.shape
    pd = torch.from_numpy(np.ascontiguousarray(part)).cuda()
    sizes = (b * hw * m * m, b * hw * m, b * m * m, b * m, b * n * 3)
    bufs = [_guarded(k) for k in sizes]
    rc = L.lns_op_letkf_combine(pd.data_ptr(), b, n, m, grid[0], grid[1], radius, bc[0], bc[1], *[v.data_ptr() for _, v in bufs], _stream())
    assert rc == 0, (rc, L.lns_create_error())
    torch.cuda.synchronize()
    for (buf, view), k in zip(bufs, sizes):
        assert _guards_intact(buf, k) and not bool((view == DSENTINEL).any())
    shapes = ((b, hw, m, m), (b, hw, m), (b, m, m), (b, m), (b, n, 3))
    return [v.view(s).cpu().numpy() for (_, v), s in zip(bufs, shapes)]


@pytest.mark.parametrize("grid", [(1, 1), (2, 2), (4, 4), (7, 15)], ids=lambda g: "%dx%d" % g)
def test_combine_op_bit_for_bit(grid):
    """Random patch sums (M = 3 and M = 33: more entries than threads), B = 2, two steps: S_l, g_l, S_glob, g_glob and stat equal the
    order-exact float64 statement bit for bit for the radii 0.5 (the own patch only), 1.0 (dist = 2 gives exactly 0) and 2.5 and
    both boundary codes per axis; S_l symmetric.  With the Gram of one patch a unit impulse the op returns the weights:
    enkf.localization_weights, bit for bit."""
    _need_gpu()
    from lns_amd import enkf
    hw = grid[0] * grid[1]
    names = ("periodic", "wall")
    for m in (3, 33):
        rng = np.random.default_rng(17 * m + hw)
        part = rng.standard_normal((2, 2, hw, m * m + m + 3)) * 10.0 ** rng.integers(-3, 4, (2, 2, hw, 1))
        for radius in (0.5, 1.0, 2.5):
            for bc in ((0, 0), (0, 1), (1, 0), (1, 1)):
                if m == 33 and bc in ((0, 1), (1, 0)) and radius != 2.5:
                    continue
                got = _combine_op(part, grid, radius, bc, m)
                want = lr.combine(part, grid, radius, bc, m)
                for name, u, v in zip(("S_local", "g_local", "S_glob", "g_glob", "stat"), got, want):
                    assert np.array_equal(u, v), (grid, m, radius, bc, name, np.abs(u - v).max())
                assert np.array_equal(got[0], got[0].transpose(0, 1, 3, 2))
    m = 2
    imp = np.zeros((hw, 1, hw, m * m + m + 3))
    imp[np.arange(hw), 0, np.arange(hw), :m * m + m] = 1.0           # sample t: patch t holds ones
    for radius in (0.5, 1.0, 2.5):
        for bc in ((0, 0), (0, 1), (1, 0), (1, 1)):
            S_l, g_l = _combine_op(imp, grid, radius, bc, m)[:2]
            want = enkf.localization_weights(grid[0], grid[1], radius, (names[bc[0]], names[bc[1]]))      # [l, t]
            for e in range(m * m):
                assert np.array_equal(S_l.reshape(hw, hw, m * m)[:, :, e].T, want), (grid, radius, bc)
            assert np.array_equal(g_l[:, :, 0].T, want)


# ---- the update op -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [2, 3, 7, 33, 64])
def test_update_op_bit_for_bit(m):
    """z [2, M, c, 3, 5] for c in {1, 8, 64, 70} (70: two channel chunks, one ragged) against the float64 numpy statement, bit for
    bit: into a separate output between guard words and in place.  With every X_l = I it equals lns_op_ensemble_transform(z, I)."""
    _need_gpu()
    from lns_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(m)
    b, h, w = 2, 3, 5
    X = rng.standard_normal((b, h * w, m, m)) + np.eye(m)
    Xd = torch.from_numpy(X).cuda()
    eye_l = torch.eye(m, dtype=torch.float64, device="cuda").expand(b, h * w, m, m).contiguous()
    eye_g = torch.eye(m, dtype=torch.float64, device="cuda").expand(b, m, m).contiguous()
    for c in (1, 8, 64, 70):
        z = (rng.standard_normal((b, m, c, h, w)) * 3.0 + 1.0).astype(np.float32)
        want = torch.from_numpy(lr.update_local(z, X)).cuda()
        zd = torch.from_numpy(z).cuda()
        n = z.size
        buf, out = _guarded(n, torch.float32)
        assert L.lns_op_ensemble_transform_local(zd.data_ptr(), Xd.data_ptr(), b, m, c, h, w, out.data_ptr(), _stream()) == 0
        torch.cuda.synchronize()
        assert _guards_intact(buf, n) and _same(out.view(z.shape), want), (m, c)
        ident = torch.empty_like(zd)
        glob = torch.empty_like(zd)
        assert L.lns_op_ensemble_transform_local(zd.data_ptr(), eye_l.data_ptr(), b, m, c, h, w, ident.data_ptr(), _stream()) == 0
        assert L.lns_op_ensemble_transform(zd.data_ptr(), eye_g.data_ptr(), b, m, c * h * w, glob.data_ptr(), _stream()) == 0
        torch.cuda.synchronize()
        assert _same(ident, glob), (m, c, "identity")
        assert L.lns_op_ensemble_transform_local(zd.data_ptr(), Xd.data_ptr(), b, m, c, h, w, zd.data_ptr(), _stream()) == 0
        torch.cuda.synchronize()
        assert _same(zd, want), (m, c, "in place")


# ---- the engine ----------------------------------------------------------------------------------------------------------------
FIELDS = ("z", "param", "X_local", "wbar_local", "lam_local", "status_local", "X", "wbar", "lam", "stat", "status", "mean", "var", "z_last")
RADIUS = 1.5
KEEPS = ([6], [1, 4, 6], [0, 1, 2, 3, 4, 5, 6])
_refs = {}


def _boundary(eng):
    from lns_amd import metrics
    return tuple(metrics.FLOW_BOUNDARIES[k] for k in metrics.flow_boundary("auto", eng.cfg))


def _want(name, steps, keep, radius=RADIUS, with_norm=True):
    """The ops on the member fields rollout_latent at batch B * M with keep_steps produces; mean / var / z_last: the shared
    reference of tests/test_etkf_gpu.py (rollout_latent_ensemble's bits); once per (case, steps, keep, radius, norm)."""
    args, model, eng, xd, z, pd, norm, y, rinv, _ = eg._case(name)
    key = (name, steps, tuple(keep), radius, with_norm)
    if key not in _refs:
        base = eg._want(name, steps, keep, with_norm)
        eg._options(eng)
        kept, zl = eng.rollout_latent(z.view((B * M,) + tuple(z.shape[2:])), steps, param=None if pd is None else pd.reshape(-1),
                                      keep_steps=keep)
        frames = kept.view((B, M) + tuple(kept.shape[1:])).permute(2, 0, 1, 3, 4, 5).contiguous()      # [n, B, M, C, Ly, Lx]
        c, h, w = (int(v) for v in z.shape[2:])
        part = eng.ensemble_patch_gram(frames, y[:, keep].contiguous(), rinv[:, keep].contiguous(), (h, w), **(norm if with_norm else {}))
        S_l, g_l, S_g, g_g, stat = eng.letkf_combine(part, (h, w), radius, _boundary(eng))
        Xl, wl, ll, sl = eng.etkf_transform(S_l.view(B * h * w, 1, M, M), g_l.view(B * h * w, 1, M), RHO)
        X, wbar, lam, status = eng.etkf_transform(S_g[:, None].contiguous(), g_g[:, None].contiguous(), RHO)
        Xl = Xl.view(B, h * w, M, M)
        za = eng.ensemble_transform_local(zl.view(z.shape).contiguous(), Xl)
        pa = eng.ensemble_transform(pd, X) if pd is not None else None
        torch.cuda.synchronize()
        assert bool((sl == 0).all()) and bool((status == 0).all())
        _refs[key] = dict(z=za, param=pa, X_local=Xl, wbar_local=wl.view(B, h * w, M), lam_local=ll.view(B, h * w, M),
                          status_local=sl.view(B, h * w), X=X, wbar=wbar, lam=lam, stat=stat, status=status, mean=base["mean"],
                          var=base["var"], z_last=base["z_last"])
    return _refs[key]


def _check(name, steps, keep, radius=RADIUS, with_norm=True, outputs=True, twice=False):
    args, model, eng, xd, z, pd, norm, y, rinv, _ = eg._case(name)
    opts = dict(eng.options)
    want = _want(name, steps, keep, radius, with_norm)
    eg._options(eng, **{k: opts.get(k, eg.DEFAULTS[k]) for k in eg.DEFAULTS})
    for _ in range(2 if twice else 1):
        got = eng.rollout_latent_ensemble_analysis_local(z, y[:, keep].contiguous(), rinv[:, keep].contiguous(), steps, radius, param=pd,
                                                         keep_steps=keep, rho=RHO, return_mean=outputs, return_var=outputs,
                                                         return_last=outputs, **(norm if with_norm else {}))
        torch.cuda.synchronize()
        tag = (name, keep, with_norm, eng.options)
        for f in FIELDS:
            u, v = getattr(got, f), want[f]
            if f in ("mean", "var", "z_last") and not outputs:
                assert u is None, tag + (f,)
            elif v is None:
                assert u is None, tag + (f,)
            elif f in ("status", "status_local"):
                assert torch.equal(u, v), tag + (f,)
            else:
                assert _same(u, v), tag + (f,)
    return got


@pytest.mark.parametrize("case,dg,ds,ov", eg.GRID)
def test_engine_call_is_the_ops_on_the_member_rollouts(case, dg, ds, ov):
    """Every output of the call == lns_op_ensemble_patch_gram, lns_op_letkf_combine, lns_op_etkf_transform (per domain and global),
    lns_op_ensemble_transform_local and lns_op_ensemble_transform (param) on rollout_latent(z.view(B * M, ...), T, keep_steps)
    arranged as [n][B][M], bit for bit, for every scheduling option (ns2d_mini) and at the defaults (the other two); mean, var
    and z_last are rollout_latent_ensemble's bits.  twophase_cond is the wall family and runs with one parameter value per
    member, which the global transform updates; sw_half_periodic has a wall in y and wraps in x."""
    _need_gpu()
    eng = eg._case(case)[2]
    try:
        for keep in KEEPS:
            _want(case, T, keep)
            if dg is not None:
                eg._options(eng, decode_group=dg, decode_streams=ds, overlap=ov)
            got = _check(case, T, keep)
            assert (got.param is not None) == (case == "twophase_cond")
    finally:
        eg._options(eng)
    assert _boundary(eng) == dict(ns2d_mini=("periodic", "periodic"), twophase_cond=("wall", "wall"),
                                  sw_half_periodic=("wall", "periodic"))[case]


def test_local_analysis_without_norm_twice_and_in_the_diagnostic_modes():
    """Without a norm; without mean / var / z_last (the update then runs in place on z_analysis); twice in a row on one workspace;
    trace and timing modes (everything on the caller's stream); lns_check_finite covers the call; the global analysis and
    rollout_latent_ensemble before and after the call return the same bits; a short workspace is refused before any work."""
    _need_gpu()
    from lns_amd import _lib
    args, model, eng, xd, z, pd, norm, y, rinv, _ = eg._case("ns2d_mini")
    keep = [1, 4, 6]
    try:
        eg._options(eng)
        before = eng.rollout_latent_ensemble(z, T, keep_steps=keep)
        _check("ns2d_mini", T, keep, with_norm=False)
        _check("ns2d_mini", T, keep, outputs=False, twice=True)
        _check("ns2d_mini", T, keep, twice=True)
        _check("ns2d_mini", T, keep, radius=0.5)
        eg._check("ns2d_mini", T, keep)                # the global filter, on the workspace the local call just used
        after = eng.rollout_latent_ensemble(z, T, keep_steps=keep)
        torch.cuda.synchronize()
        assert _same(before[0], after[0]) and _same(before[1], after[1])
        eng.check_finite(B * M, z.device)
        eg._options(eng, decode_group=2)
        eng.timing_enable(True)
        _check("ns2d_mini", T, keep)
        eng.timing_enable(False)
        eng.trace_enable(True)
        _check("ns2d_mini", T, keep)
        eng.trace_enable(False)
    finally:
        eng.timing_enable(False)
        eng.trace_enable(False)
        eg._options(eng)
    L, h = eng._L, eng._h
    n0, n1, n2 = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert L.lns_rollout_ensemble_workspace_bytes(h, B, M, ctypes.byref(n0)) == 0
    assert L.lns_rollout_ensemble_analysis_local_workspace_bytes(h, B, M, 3, ctypes.byref(n1)) == 0
    assert L.lns_rollout_ensemble_analysis_local_workspace_bytes(h, B, M, 4, ctypes.byref(n2)) == 0
    c, lh, lw = (int(v) for v in z.shape[2:])
    patch_sums = B * lh * lw * (M * M + M + 3) * 8
    assert n1.value - n0.value >= 3 * patch_sums and patch_sums <= n2.value - n1.value <= patch_sums + 1024
    za = torch.full_like(z, DSENTINEL)
    ws = torch.empty(n1.value, dtype=torch.uint8, device="cuda")
    yk, rk = y[:, keep].contiguous(), rinv[:, keep].contiguous()
    per = yk[0, 0].numel()

    def run(nbytes):
        return L.lns_rollout_latent_ensemble_analysis_local(h, z.data_ptr(), None, yk.data_ptr(), rk.data_ptr(), 3 * per, per, B, M, T,
                                                            (ctypes.c_int * 3)(*keep), 3, None, RHO, RADIUS, 0, 0, za.data_ptr(), None, None,
                                                            None, None, None, None, None, None, None, None, None, None, None,
                                                            ws.data_ptr(), nbytes, _stream())
    for short in (n1.value - 1, n0.value):
        assert run(short) == _lib.LNS_ENOMEM and "local ensemble analysis workspace too small" in L.lns_last_error(h).decode()
        torch.cuda.synchronize()
        assert bool((za == DSENTINEL).all())
    assert run(n1.value) == 0
    torch.cuda.synchronize()
    assert _same(za, _want("ns2d_mini", T, keep, with_norm=False)["z"])


def test_locality_on_the_device():
    """ns2d_mini, rho = 1, the observations confined to one patch, radius 0.5 (the own patch only): the latents of every other pixel
    equal lns_op_ensemble_transform(z_last, I) bit for bit (X_l = I exactly, wbar = 0), and the observed pixel's do not."""
    _need_gpu()
    args, model, eng, xd, z, pd, norm, y, rinv, _ = eg._case("ns2d_mini")
    eg._options(eng)
    c, h, w = (int(v) for v in z.shape[2:])
    pidx = torch.from_numpy(lr.patch_index(args.Ly, args.Lx, h, w)).cuda()
    own = (h // 2) * w + w // 3
    keep = [2, 5]
    r = torch.where(pidx == own, torch.full((), 2.0, device="cuda"), torch.zeros((), device="cuda")).expand(args.in_channels, -1, -1).contiguous()
    a = eng.rollout_latent_ensemble_analysis_local(z, y[:, keep].contiguous(), r, T, 0.5, keep_steps=keep, rho=1.0, return_last=True, **norm)
    eye = torch.eye(M, dtype=torch.float64, device="cuda").expand(B, M, M).contiguous()
    kept = eng.ensemble_transform(a.z_last.contiguous(), eye)
    torch.cuda.synchronize()
    assert bool((a.status_local == 0).all()) and float(a.stat[:, :, 2].min()) > 0
    got, want = a.z.reshape(B, M, c, h * w), kept.reshape(B, M, c, h * w)
    others = torch.arange(h * w, device="cuda") != own
    assert _same(got[..., others].contiguous(), want[..., others].contiguous())
    assert not _same(got[..., own].contiguous(), want[..., own].contiguous())
    Xl = a.X_local.view(B, h * w, M, M)
    assert bool((Xl[:, others] == torch.eye(M, dtype=torch.float64, device="cuda")).all()) and not bool(a.wbar_local[:, others].any())
    assert bool((a.wbar_local[:, own] != 0).any())


# ---- the filter and the drop-in ---------------------------------------------------------------------------------------------------
def test_local_filter_cycles_windows_from_the_previous_analysis():
    """LocalEnsembleFilter.run with window = 1 over two observed steps == two calls by hand, the second from the first one's
    analysis; window = 2 == one call; dfs per domain from lam_local; keep_X = False drops X."""
    _need_gpu()
    from lns_amd import enkf
    args, model, eng, xd, z, pd, norm, y, rinv, _ = eg._case("ns2d_mini")
    eg._options(eng)
    obs = [1, 4]
    yk, rk = y[:, obs].contiguous(), rinv[:, obs].contiguous()
    f = enkf.LocalEnsembleFilter(model, RADIUS, inflation=RHO)
    got = f.run(z, yk, rk, obs, window=1, **norm)
    a = eng.rollout_latent_ensemble_analysis_local(z, yk[:, :1].contiguous(), rk[:, :1].contiguous(), 2, RADIUS, keep_steps=[1], rho=RHO, **norm)
    b = eng.rollout_latent_ensemble_analysis_local(a.z, yk[:, 1:].contiguous(), rk[:, 1:].contiguous(), 3, RADIUS, keep_steps=[2], rho=RHO, **norm)
    torch.cuda.synchronize()
    assert isinstance(got, enkf.LocalEnKFResult)
    assert _same(got.z, b.z) and _same(got.X, torch.stack([a.X_local, b.X_local])) and _same(got.stat, torch.cat([a.stat, b.stat], 1))
    hw = a.lam_local.shape[1]
    assert tuple(got.dfs.shape) == (2, B, hw) and bool((got.dfs > -1e-12).all()) and bool((got.dfs < M - 1).all()) and got.param is None
    assert torch.allclose(got.dfs[1], (1.0 - (M - 1) / (RHO * b.lam_local)).sum(-1), rtol=0, atol=1e-12)
    assert torch.equal(got.status, torch.stack([a.status_local, b.status_local]))
    both = enkf.LocalEnsembleFilter(model, RADIUS, inflation=RHO, keep_X=False).run(z, yk, rk, obs, window=2, **norm)
    one = eng.rollout_latent_ensemble_analysis_local(z, yk, rk, 5, RADIUS, keep_steps=obs, rho=RHO, **norm)
    torch.cuda.synchronize()
    assert _same(both.z, one.z) and both.X is None and _same(both.lam[0], one.lam_local) and tuple(both.status.shape) == (1, B, hw)
    single = f.analysis(z, yk, rk, 5, obs, **norm)
    torch.cuda.synchronize()
    assert _same(single.z, one.z) and _same(single.X[0], one.X_local)


def test_drop_in_takes_loc_radius_and_keeps_todays_bits_without_it():
    """assimilate_ensemble(loc_radius=1.0) returns LocalEnKFResult, equal to LocalEnsembleFilter.run on the members it draws; without
    loc_radius (and with loc_radius=None) it returns EnKFResult with the bits of EnsembleFilter.run on the same members."""
    _need_gpu()
    import gpu_checks as gc
    from helpers import load_golden, case_args
    from lns_amd import enkf, filler
    t = er.TWIN
    meta, _ = load_golden(t["preset"])
    args = case_args(meta)
    model, _ = gc.build_models(args, meta["weight_seed"])
    tail = (args.in_channels, args.Ly, args.Lx)
    x0 = torch.from_numpy(filler.normal("x", (t["B"],) + tail, t["x_seed"])).cuda()
    eng = model._engine(x0)
    obs = list(t["obs_steps"])
    truth, _ = eng.rollout_latent(model.x_to_z(x0), obs[-1] + 1, keep_steps=obs)
    truth = truth.contiguous()
    r = torch.from_numpy(er.twin_rinv(*tail, t["rinv"])).cuda()

    def gen():
        g = torch.Generator(device="cuda")
        g.manual_seed(t["gpu_seed"])
        return g
    zm = model._ensemble_latents(x0, t["M"], t["noise_level"], gen(), False).contiguous()
    plain = model.assimilate_ensemble(x0, truth, obs, t["M"], t["noise_level"], rinv=r, generator=gen())
    none = model.assimilate_ensemble(x0, truth, obs, t["M"], t["noise_level"], rinv=r, generator=gen(), loc_radius=None)
    want = enkf.EnsembleFilter(model, 1.0).run(zm, truth, r, obs)
    local = model.assimilate_ensemble(x0, truth, obs, t["M"], t["noise_level"], rinv=r, generator=gen(), loc_radius=1.0)
    lwant = enkf.LocalEnsembleFilter(model, 1.0, 1.0, "auto").run(zm, truth, r, obs)
    torch.cuda.synchronize()
    assert type(plain) is enkf.EnKFResult and type(none) is enkf.EnKFResult and type(local) is enkf.LocalEnKFResult
    for f in ("z", "X", "lam", "stat", "dfs"):
        assert _same(getattr(plain, f), getattr(want, f)) and _same(getattr(none, f), getattr(want, f)), f
        assert _same(getattr(local, f), getattr(lwant, f)), f
    assert bool((local.status == 0).all()) and local.X.dim() == 5 and not _same(local.z, plain.z)

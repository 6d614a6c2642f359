"""GPU (-m gpu): the Python side of the six ensemble rollout methods of `Engine` (rollout_latent_ensemble and its _eval,
_quantiles, _exceed, _analysis and _analysis_local forms) and of the four op wrappers that take frames and a truth
(ensemble_score, ensemble_exceed, ensemble_obs_gram, ensemble_patch_gram): the text of every refusal they decide themselves,
which of two failing checks answers, which of mean / var / z_last are None under every combination of the return flags, and the
shapes and dtypes of everything a call with all flags on returns.  ns2d_mini at B = 2, M = 3, T = 3, keep_steps = [0, 2].  A
device is needed only because the wrappers refuse CPU tensors first: the refusals launch nothing."""
import pytest

torch = pytest.importorskip("torch")

import test_etkf_gpu as eg  # noqa: E402

pytestmark = pytest.mark.gpu

B, M, T, KEEP = eg.B, eg.M, 3, [0, 2]
NK = len(KEEP)
FORMS = ("plain", "eval", "quantiles", "exceed", "analysis", "local")
TRUTH = {"eval": "y", "exceed": "y", "analysis": "y_obs", "local": "y_obs"}       # the form's truth argument
VAR_NEEDS_MEAN = "return_var needs return_mean (the variance comes from the kernel that writes the mean)"
NO_CPU = "the LNS engine runs on HIP device tensors only (got cpu); there is no CPU fallback"
NO_F64 = "fp32 tensors expected, got torch.float64"
KEEP_2_0 = "keep_steps must be ascending steps in [0, 3): entry 1 is 0"
MEMBERS_2_64 = "ensemble analysis needs M in 2 .. 64 (the transform keeps A and Q in LDS; 65 .. 128 members are not supported)"


def _case():
    """(engine, cfg, latent shape, z [B, M, c, h, w], y [B, T, C, Ly, Lx], rinv [B, NK, C, Ly, Lx]) of tests/test_etkf_gpu.py's
    ns2d_mini case; nothing here writes them"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    args, model, eng, xd, z, pd, norm, y, rinv, _ = eg._case("ns2d_mini")
    return eng, eng.cfg, eng.latent_shape(), z, y[:, :T].contiguous(), rinv[:, KEEP].contiguous()


def _call(form, z=None, y=None, y_obs=None, rinv=None, steps=T, keep_steps=KEEP, **kw):
    """one call of the form's method on the case's inputs, with what the keywords replace"""
    eng, cfg, lat, z0, y0, r0 = _case()
    z = z0 if z is None else z
    y = y0 if y is None else y
    y_obs = y0[:, KEEP].contiguous() if y_obs is None else y_obs
    rinv = r0 if rinv is None else rinv
    if form == "plain":
        return eng.rollout_latent_ensemble(z, steps, keep_steps=keep_steps, **kw)
    if form == "eval":
        return eng.rollout_latent_ensemble_eval(z, y, steps, keep_steps=keep_steps, **kw)
    if form == "quantiles":
        return eng.rollout_latent_ensemble_quantiles(z, steps, kw.pop("quantiles", (0.25, 0.5)), kw.pop("thresholds", (0.1,)),
                                                     keep_steps=keep_steps, **kw)
    if form == "exceed":
        return eng.rollout_latent_ensemble_exceed(z, y, steps, kw.pop("thresholds", (0.1, 0.2)), keep_steps=keep_steps, **kw)
    if form == "analysis":
        return eng.rollout_latent_ensemble_analysis(z, y_obs, rinv, steps, keep_steps=keep_steps, **kw)
    return eng.rollout_latent_ensemble_analysis_local(z, y_obs, rinv, steps, 2.0, keep_steps=keep_steps, **kw)


def _refused(text, form, exc=None, **kw):
    from lns_amd._lib import LnsError
    with pytest.raises(exc or LnsError) as info:
        _call(form, **kw)
    assert str(info.value) == text, (form, kw.keys())


@pytest.mark.parametrize("form", FORMS)
def test_latents_of_the_wrong_rank_or_tail_are_refused_first(form):
    eng, cfg, (c, h, w), z, y, rinv = _case()
    text = "ensemble latents must be [B, M, %d, %d, %d], got %%s" % (c, h, w)
    flat, cut = z[:, 0].contiguous(), z[..., :-1]
    _refused(text % (tuple(flat.shape),), form, z=flat)
    _refused(text % (tuple(cut.shape),), form, z=cut)
    _refused(NO_CPU, form, z=z.cpu())
    _refused(NO_F64, form, z=z.double())
    # two failing checks: the latents answer before the return flags, the truth's shape, the steps, keep_steps and param
    bad = dict(return_var=True) if form != "plain" else {}
    _refused(text % (tuple(flat.shape),), form, z=flat, keep_steps=[2, 0], param=torch.zeros(5, device=z.device), **bad)
    if form in TRUTH:
        _refused(text % (tuple(cut.shape),), form, z=cut, **{TRUTH[form]: y[:, :, :, :-1]})
        _refused(NO_CPU, form, z=z.cpu(), **{TRUTH[form]: y.double()})             # (both pass _dev, the latents first)


@pytest.mark.parametrize("form", FORMS)
def test_return_flags_member_count_steps_and_param_are_refused_in_order(form):
    eng, cfg, (c, h, w), z, y, rinv = _case()
    dev = z.device
    one = z[:, :1].contiguous()
    five = torch.zeros(5, device=dev)
    PARAM = "param must hold one value per trajectory or per member: got 5 values for B = 2, M = 3"
    if form == "plain":
        m1 = "the variance needs at least 2 members, got M = 1 (return_var=False for the mean alone)"
        _refused(m1, form, z=one)
        _refused(m1, form, z=one, keep_steps=[2, 0], out=torch.empty(3, device=dev), param=five)
        shape = (B, NK, cfg.in_channels, cfg.Ly, cfg.Lx)
        _refused("preallocated output must be contiguous with shape %s" % (shape,), form, out=torch.empty(3, device=dev), param=five)
        _refused(KEEP_2_0, form, keep_steps=[2, 0], out=torch.empty(3, device=dev))
    else:
        _refused(VAR_NEEDS_MEAN, form, return_var=True)
        _refused(VAR_NEEDS_MEAN, form, return_var=True, return_last=True, param=five)
    if form in ("quantiles", "exceed"):
        m1 = "the variance needs at least 2 members, got M = 1"
        _refused(m1, form, z=one, return_mean=True, return_var=True)
        _refused(VAR_NEEDS_MEAN, form, z=one, return_var=True)                      # before the member count
        _refused(m1, form, z=one, return_mean=True, return_var=True, keep_steps=[2, 0])
    if form == "eval":                                                              # no check of its own: the library answers
        _refused("lns_rollout_latent_ensemble_eval failed (-1): var_out needs M >= 2", form, z=one, return_mean=True, return_var=True)
    if form in ("analysis", "local"):                                               # likewise, in the size query
        query = "lns_rollout_ensemble_analysis%s_workspace_bytes" % ("_local" if form == "local" else "")
        _refused("%s failed (-1): %s" % (query, MEMBERS_2_64), form, z=one, return_mean=True, return_var=True)
    if form in ("eval", "exceed"):
        fit = "4 steps do not fit the 3 steps of the ground truth"
        _refused(fit, form, steps=T + 1)
        _refused(fit, form, steps=T + 1, keep_steps=[2, 0], param=five)
        _refused(VAR_NEEDS_MEAN, form, steps=T + 1, return_var=True)                # the flags before the steps
    _refused(KEEP_2_0, form, keep_steps=[2, 0])
    _refused(KEEP_2_0, form, keep_steps=[2, 0], param=five)
    _refused(PARAM, form, param=five)
    _refused("param is on cpu but the latents are on %s" % dev, form, param=torch.zeros(B))
    # the form's own request is looked at before param
    if form == "quantiles":
        _refused("neither a quantile nor a threshold was asked for", form, ValueError, quantiles=(), thresholds=(), param=five)
        _refused(KEEP_2_0, form, keep_steps=[2, 0], quantiles=(), thresholds=())
    if form == "exceed":
        _refused("between 1 and 8 thresholds per call, got 0", form, ValueError, thresholds=(), param=five)
    if form in ("analysis", "local"):
        tail = (cfg.in_channels, cfg.Ly, cfg.Lx)
        r = rinv[:, :1]
        text = "rinv must be %s, %s or %s, got %s" % (tail, (NK,) + tail, (B, NK) + tail, tuple(r.shape))
        _refused(text, form, rinv=r, param=five)
        _refused(VAR_NEEDS_MEAN, form, rinv=r, return_var=True)
        _refused("rinv must be an fp32 HIP tensor on the device of the fields", form, rinv=rinv.cpu(), param=five)


@pytest.mark.parametrize("form", sorted(TRUTH))
def test_a_truth_of_the_wrong_shape_dtype_or_device_is_refused(form):
    eng, cfg, (c, h, w), z, y, rinv = _case()
    name = TRUTH[form]
    tail = (cfg.in_channels, cfg.Ly, cfg.Lx)
    _refused(NO_CPU, form, **{name: y.cpu()})
    _refused(NO_F64, form, **{name: y.double()})
    if name == "y":
        text = "ground truth must be fp32 [B, T, %d, %d, %d] with the latents' batch, got %%s" % tail
        for bad in (y[:, :, :, :-1], y[:1], y[:, 0], y[:, :, :1]):
            _refused(text % (tuple(bad.shape),), form, y=bad)
        _refused(text % (tuple(y[:1].shape),), form, y=y[:1], return_var=True, steps=T + 1)       # the truth before flags and steps
    else:
        text = "y_obs must be %s on the latents' device, got %%s" % ((B, NK) + tail,)
        for bad in (y, y[:, :1], y[:1, KEEP], y[:, KEEP][..., :-1], y[:, 0]):
            _refused(text % (tuple(bad.shape),), form, y_obs=bad)
        _refused(text % (tuple(y.shape),), form, y_obs=y, return_var=True, rinv=rinv[:, :1])         # the truth before flags and rinv
        _refused(KEEP_2_0, form, y_obs=y, keep_steps=[2, 0])                                       # keep_steps before the truth


def _fields(form, res, return_var, return_last):
    """(mean, var, z_last, {every other field}) of a result"""
    if form == "plain":
        res = res if isinstance(res, tuple) else (res,)
        assert len(res) == 1 + int(return_var) + int(return_last)
        return res[0], res[1] if return_var else None, res[-1] if return_last else None, {}
    d = res._asdict()
    return d.pop("mean"), d.pop("var"), d.pop("z_last"), d


@pytest.mark.parametrize("form", FORMS)
def test_what_is_returned_under_every_combination_of_the_flags(form):
    """mean / var / z_last are tensors of the documented shape exactly where asked for and None elsewhere; the form's own fields
    have their documented shapes and dtypes under all of them"""
    eng, cfg, (c, h, w), z, y, rinv = _case()
    C, hw = cfg.in_channels, h * w
    field = (B, NK, C, cfg.Ly, cfg.Lx)
    f32, f64, i32 = torch.float32, torch.float64, torch.int32
    glob = dict(z=(tuple(z.shape), f32), param=None, X=((B, M, M), f64), wbar=((B, M), f64), lam=((B, M), f64), stat=((B, NK, 3), f64),
                status=((B,), i32))
    own = {"plain": {},
           "eval": dict(rel_l2=((B, NK, C), f32), rmse=((B, NK, C), f32), spread=((B, NK, C), f32), crps=((B, NK, C), f32),
                        seq=((B, C, 4), f32), rank=((B, NK, C, M + 1), i32)),
           "quantiles": dict(quantiles=((B, NK, 2) + field[2:], f32), prob=((B, NK, 1) + field[2:], f32)),
           "exceed": dict(table=((B, NK, 2, C, 2, M + 1), i32)),
           "analysis": glob,
           "local": dict(glob, X_local=((B, hw, M, M), f64), wbar_local=((B, hw, M), f64), lam_local=((B, hw, M), f64),
                         status_local=((B, hw), i32))}[form]
    if form == "plain":
        combos = [(True, v, l) for v in (False, True) for l in (False, True)]
    else:
        combos = [(m, v, l) for m, v in ((False, False), (True, False), (True, True)) for l in (False, True)]
    for want_mean, want_var, want_last in combos:
        flags = dict(return_var=want_var, return_last=want_last)
        if form != "plain":
            flags["return_mean"] = want_mean
        res = _call(form, **flags)
        if form == "plain" and not want_var and not want_last:
            assert isinstance(res, torch.Tensor)
        mean, var, z_last, rest = _fields(form, res, want_var, want_last)
        for t, want, shape in ((mean, want_mean, field), (var, want_var, field), (z_last, want_last, tuple(z.shape))):
            assert (t is not None) == want, (form, flags)
            if want:
                assert tuple(t.shape) == shape and t.dtype == f32 and t.device == z.device and t.is_contiguous(), (form, flags)
        assert set(rest) == set(own), form
        for k, spec in own.items():
            if spec is None:
                assert rest[k] is None, (form, k)
            else:
                assert tuple(rest[k].shape) == spec[0] and rest[k].dtype == spec[1] and rest[k].device == z.device, (form, k, flags)
    torch.cuda.synchronize()
    if form == "plain":                                                            # out=: the caller's mean comes back
        out = torch.empty(field, device=z.device)
        assert _call(form, return_var=False, out=out) is out
    if form == "eval":
        assert _call(form, return_rank=False).rank is None
    if form == "quantiles":
        q = _call(form, thresholds=())
        assert q.prob is None and q.quantiles is not None
        q = _call(form, quantiles=())
        assert q.quantiles is None and q.prob is not None
    if form == "local":
        r = _call(form, return_X=False)
        assert r.X_local is None and r.wbar_local is None and tuple(r.lam_local.shape) == (B, hw, M)
    torch.cuda.synchronize()


OPS = (("ensemble_score", "y"), ("ensemble_exceed", "y"), ("ensemble_obs_gram", "y_obs"), ("ensemble_patch_gram", "y_obs"))


@pytest.mark.parametrize("op,yname", OPS)
def test_the_op_wrappers_refuse_frames_and_truth_that_do_not_fit(op, yname):
    from lns_amd._lib import LnsError
    eng, cfg, (c, h, w), z, y, rinv = _case()
    n, C, H, W = 3, 2, 4, 5
    frames = torch.zeros((n, B, M, C, H, W), device=z.device)
    truth = torch.zeros((B, n, C, H, W), device=z.device)
    r = torch.ones((C, H, W), device=z.device)

    def call(f, t):
        if op == "ensemble_score":
            return eng.ensemble_score(f, t)
        if op == "ensemble_exceed":
            return eng.ensemble_exceed(f, t, (0.1,))
        if op == "ensemble_obs_gram":
            return eng.ensemble_obs_gram(f, t, r)
        return eng.ensemble_patch_gram(f, t, r, (2, 2))
    kinds = "%s takes fp32 HIP tensors" % op
    dims = "%s takes frames [n, B, M, C, H, W] and %s [B, n, C, H, W] on one device" % (op, yname)
    cases = [(frames.cpu(), truth, kinds), (frames, truth.cpu(), kinds), (frames.double(), truth, kinds), (frames, truth.double(), kinds),
             (frames.cpu(), truth[0], kinds),                                       # two failing checks: the kind before the rank
             (None, truth, kinds), (frames[0], truth, dims), (frames, truth[0], dims),
             (frames[0], truth[:, :1], dims)]                                       # the rank before the shape
    for bad in (truth[:, :1], truth[:1], truth[..., :-1], truth.transpose(0, 1)):
        if tuple(bad.shape) != tuple(truth.shape):
            cases.append((frames, bad, "%s must be %s for frames %s, got %s" % (yname, (B, n, C, H, W), tuple(frames.shape), tuple(bad.shape))))
    for f, t, text in cases:
        with pytest.raises(LnsError) as info:
            call(f, t)
        assert str(info.value) == text, (op, text)
    call(frames, truth)                                                             # and what fits is accepted
    torch.cuda.synchronize()

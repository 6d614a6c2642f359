"""Validation-loop helpers next to the hot path: fused denormalise + relative-L2 metric, bulk
dataset encode.  Mirrors the reference call sites:

    y_hat = val_dataset.denormalize(model.predict(x, T, to_x=True)); y = val_dataset.denormalize(y)
    frame_wise = relative_lp_loss(y_hat, y, reduce_dim=(3, 4), p=2)        # train_stage2_ns2d.py:253-257
    seq_wise   = relative_lp_loss(y_hat, y, reduce_dim=(1, 3, 4), p=2)
    dataset.encode_dataset(vq_ae, device)                                   # ns2d_fno_stage2_simpleae.py:81-93

The other datasets' denormalize() (per-channel statistics, dataset/Stage2_SW.py:60-72; closed-tank wall velocities
zeroed and VOF clamped, dataset/twophase_flow_stage2.py:370-390) are the same kernel with a per-channel spec:
`relative_l2(..., mean=[...], std=[...], zero_wall_channels=(0, 1), clamp_channels=(3,))` or `twophase_spec(...)`.
"""
import collections
import ctypes

import torch

from . import _lib


def twophase_spec(vel_mean, vel_std, prs_mean, prs_std):
    """Keyword arguments for relative_l2 that restate TwoPhaseFlow dataset denormalisation
    (dataset/twophase_flow_stage2.py:370-390): channels (u, v, p, vof)."""
    return dict(mean=[vel_mean, vel_mean, prs_mean, 0.0], std=[vel_std, vel_std, prs_std, 1.0],
                zero_wall_channels=(0, 1), clamp_channels=(3,), clamp=(0.0, 1.0 + 1e-8))


def relative_l2(y_hat, y, mean=0.0, std=1.0, eps=1e-8, zero_wall_channels=(), clamp_channels=(), clamp=(0.0, 1.0 + 1e-8)):
    """(frame_wise [B,T,C], seq_wise [B,C]) relative L2 errors of a normalised rollout y_hat against the normalised
    ground truth y, both [B,T,C,H,W], after the dataset's denormalisation: x*std + mean with scalar or per-channel
    statistics, optionally the wall rows/columns of `zero_wall_channels` zeroed and `clamp_channels` clamped.
    One HIP pass over both tensors; CPU tensors raise -- there is no CPU fallback."""
    if not (y_hat.is_cuda and y.is_cuda):
        raise RuntimeError("lns_amd.metrics.relative_l2 needs CUDA/HIP tensors (no CPU fallback)")
    if y_hat.shape != y.shape or y_hat.dim() != 5:
        raise ValueError("expected two [B,T,C,H,W] tensors of the same shape")
    y_hat = y_hat.contiguous().float()
    y = y.contiguous().float()
    B, T, C, H, W = y.shape
    frame = torch.empty((B, T, C), dtype=torch.float32, device=y.device)
    seq = torch.empty((B, C), dtype=torch.float32, device=y.device)
    scratch = torch.empty((B * T * C * 2,), dtype=torch.float32, device=y.device)
    if y_hat.device != y.device:
        raise ValueError("y_hat is on %s but y is on %s" % (y_hat.device, y.device))
    L = _lib.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream(y.device).cuda_stream)
    per_channel = (not isinstance(mean, (int, float))) or (not isinstance(std, (int, float))) or \
        len(zero_wall_channels) > 0 or len(clamp_channels) > 0
    # the metric entry points launch on the CURRENT device (include/lns.h): make that the tensors' device
    with torch.cuda.device(y.device):
        rc = _launch_metric(L, per_channel, y_hat, y, B, T, C, H, W, mean, std, eps, zero_wall_channels, clamp_channels,
                            clamp, frame, seq, scratch, stream)
    if rc != 0:
        raise RuntimeError("lns_metric_rel_l2 failed (rc=%d)" % rc)
    return frame, seq


def _launch_metric(L, per_channel, y_hat, y, B, T, C, H, W, mean, std, eps, zero_wall_channels, clamp_channels, clamp,
                   frame, seq, scratch, stream):
    if not per_channel:
        rc = L.lns_metric_rel_l2(y_hat.data_ptr(), y.data_ptr(), B, T, C, H * W, float(mean), float(std), float(eps),
                                 frame.data_ptr(), seq.data_ptr(), scratch.data_ptr(), stream)
    else:
        def per_c(v):
            v = [float(v)] * C if isinstance(v, (int, float)) else [float(e) for e in v]
            if len(v) != C:
                raise ValueError("per-channel statistics need %d entries" % C)
            return (ctypes.c_float * C)(*v)
        flags = [0] * C
        for c in zero_wall_channels:
            flags[c] |= 1
        for c in clamp_channels:
            flags[c] |= 2
        m, sd, fl = per_c(mean), per_c(std), (ctypes.c_int * C)(*flags)
        rc = L.lns_metric_rel_l2_ch(y_hat.data_ptr(), y.data_ptr(), B, T, C, H, W, m, sd, fl, float(clamp[0]),
                                    float(clamp[1]), float(eps), frame.data_ptr(), seq.data_ptr(),
                                    scratch.data_ptr(), stream)
    return rc


SPECTRUM_BASES = ("dft", "dct")


def spectrum_basis(basis, cfg=None):
    """(basis_y, basis_x) as LNS_SPECTRUM_DFT / LNS_SPECTRUM_DCT (0 / 1) from "dft", "dct", a pair (y, x) of the two names, or
    "auto": per axis "dft" where the model's autoencoder pads that axis circularly (cfg.ae_pad_y / ae_pad_x of an engine's
    configuration), else "dct" -- dft / dft for ns2d*, dct / dft for sw_half_periodic, dct / dct for the two-phase presets.
    Host only; anything else raises LnsError."""
    def one(b):
        if not isinstance(b, str) or b not in SPECTRUM_BASES:
            raise _lib.LnsError('spectrum basis: "dft", "dct", a pair (y, x) of them or "auto", got %r' % (basis,))
        return SPECTRUM_BASES.index(b)
    if isinstance(basis, str):
        if basis == "auto":
            if cfg is None:
                raise _lib.LnsError('spectrum basis "auto" needs a model (Engine.energy_spectrum / the rollout calls): '
                                    'name the basis of stored fields')
            return tuple(0 if pad == _lib.LNS_PAD_CIRCULAR else 1 for pad in (cfg.ae_pad_y, cfg.ae_pad_x))
        return one(basis), one(basis)
    try:
        by, bx = basis
    except (TypeError, ValueError):
        raise _lib.LnsError('spectrum basis: "dft", "dct", a pair (y, x) of them or "auto", got %r' % (basis,))
    return one(by), one(bx)


def spectrum_bins(H, W, basis="dft"):
    """Number of shells S of the energy spectrum of an H x W plane (include/lns.h "energy spectra"): the shell of the
    corner mode plus one -- (H/2, W/2) for dft / dft, else in half cycles per side (`spectrum_wavenumbers`).  Host only; an
    unsupported plane (H, W <= 192 and H * W <= 18432) raises."""
    by, bx = spectrum_basis(basis)
    L = _lib.lib()
    S = L.lns_spectrum_bins(int(H), int(W)) if (by, bx) == (0, 0) else L.lns_spectrum_bins_basis(int(H), int(W), by, bx)
    if S < 0:
        raise _lib.LnsError("energy spectrum: a %d x %d plane is not supported (H, W <= 192 and H * W <= 18432)" % (H, W))
    return int(S)


def spectrum_wavenumbers(H, W, basis="dft"):
    """Bin centres of `energy_spectrum` in cycles per side, a float64 tensor [S]: s for dft / dft, s / 2 once an axis is
    "dct" (its wavenumbers count half cycles)."""
    by, bx = spectrum_basis(basis)
    k = torch.arange(spectrum_bins(H, W, basis), dtype=torch.float64)
    return k if (by, bx) == (0, 0) else k / 2


def energy_spectrum(y_hat, y=None, mean=0.0, std=1.0, eps=1e-8, zero_wall_channels=(), clamp_channels=(), clamp=(0.0, 1.0 + 1e-8),
                    basis="dft"):
    """Shell-summed energy spectra of stored fields (lns_op_energy_spectrum): y_hat and y (optional) [B,T,C,H,W],
    normalised, denormalised as in `relative_l2` (eps is not used).  Returns [B,T,C,3,S] -- forecast, truth and error
    (forecast - truth, differenced before the transform) -- or, without y, [B,T,C,1,S]; S = spectrum_bins(H, W, basis), bin s
    holds the energy of the modes whose index wavenumber rounds to s, and the bins of a row sum to mean(u^2).  `basis`:
    "dft" (default), "dct" or a pair (y, x).  Under "dft" an axis with walls puts the jump across them into the spectrum (a
    k^-2 tail); give such an axis "dct" (DCT-II, the DFT of the mirror extension: no jump), and read the bins with
    `spectrum_wavenumbers`.  The kernel body of Engine.rollout_eval_spectrum."""
    from .engine import eval_spec
    by, bx = spectrum_basis(basis)
    for t in (y_hat, y):
        if t is not None and (not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 5):
            raise _lib.LnsError("energy_spectrum takes fp32 HIP tensors [B,T,C,H,W] (no CPU fallback)")
    if y is not None and (y.shape != y_hat.shape or y.device != y_hat.device):
        raise _lib.LnsError("y must have y_hat's shape %s and device, got %s" % (tuple(y_hat.shape), tuple(y.shape)))
    B, T, C, H, W = (int(v) for v in y_hat.shape)
    S = spectrum_bins(H, W, SPECTRUM_BASES[by] if by == bx else (SPECTRUM_BASES[by], SPECTRUM_BASES[bx]))
    y_hat = y_hat.contiguous()
    y = y.contiguous() if y is not None else None
    spec = eval_spec(C, mean=mean, std=std, eps=eps, zero_wall_channels=zero_wall_channels, clamp_channels=clamp_channels,
                     clamp=clamp)
    out = torch.empty((B, T, C, 3 if y is not None else 1, S), dtype=torch.float32, device=y_hat.device)
    L = _lib.lib()
    with torch.cuda.device(y_hat.device):
        stream = ctypes.c_void_p(torch.cuda.current_stream(y_hat.device).cuda_stream)
        args = (y_hat.data_ptr(), y.data_ptr() if y is not None else None, B, T, C, H, W, ctypes.byref(spec), out.data_ptr(), stream)
        rc = L.lns_op_energy_spectrum(*args) if (by, bx) == (0, 0) else L.lns_op_energy_spectrum_basis(*args, by, bx)
    if rc != 0:
        raise _lib.LnsError("lns_op_energy_spectrum failed (%d): %s" % (rc, L.lns_create_error().decode()))
    return out


FIELD_STATS = ("mean_P", "mean_Q", "var_P", "var_Q", "corr", "cos", "grad_y", "grad_x", "min_P", "max_P", "min_Q", "max_Q")


def field_stats(y_hat, y, hist=None, mean=0.0, std=1.0, eps=1e-8, zero_wall_channels=(), clamp_channels=(), clamp=(0.0, 1.0 + 1e-8)):
    """Per-plane statistics of stored fields (lns_op_field_stats; include/lns.h "field statistics"): y_hat and y [B,T,C,H,W],
    normalised, denormalised as in `relative_l2` into forecast P and truth Q.  Returns (stats [B,T,C,12], hist): the columns
    are FIELD_STATS -- the means and biased variances of P and Q, their centred correlation `corr`, the reference's
    pointwise_correlation `cos`, the relative L2 of the central differences in y and x (GradientDomainLoss.spatial_fd, no
    wrap-around), and the extrema.  hist = (nbins, lo, hi) with scalar or per-channel edges adds int32 counts
    [B,T,C,2,nbins+2] (rows forecast, truth; bin 0 below lo, bin nbins+1 from hi on; see histogram_edges), else None.
    The kernel body of Engine.rollout_eval_stats."""
    from .engine import eval_spec, stats_spec
    for t in (y_hat, y):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 5:
            raise _lib.LnsError("field_stats takes fp32 HIP tensors [B,T,C,H,W] (no CPU fallback)")
    if y.shape != y_hat.shape or y.device != y_hat.device:
        raise _lib.LnsError("y must have y_hat's shape %s and device, got %s" % (tuple(y_hat.shape), tuple(y.shape)))
    B, T, C, H, W = (int(v) for v in y_hat.shape)
    y_hat, y = y_hat.contiguous(), y.contiguous()
    spec = eval_spec(C, mean=mean, std=std, eps=eps, zero_wall_channels=zero_wall_channels, clamp_channels=clamp_channels,
                     clamp=clamp)
    hs = stats_spec(C, hist)
    stats = torch.empty((B, T, C, _lib.LNS_FIELD_STATS), dtype=torch.float32, device=y_hat.device)
    counts = None
    if hs is not None:
        if not 1 <= hs.nbins <= 256:
            raise _lib.LnsError("hist: nbins must be in 1 .. 256, got %d" % hs.nbins)
        counts = torch.empty((B, T, C, 2, hs.nbins + 2), dtype=torch.int32, device=y_hat.device)
    L = _lib.lib()
    with torch.cuda.device(y_hat.device):
        stream = ctypes.c_void_p(torch.cuda.current_stream(y_hat.device).cuda_stream)
        rc = L.lns_op_field_stats(y_hat.data_ptr(), y.data_ptr(), B, T, C, H, W, ctypes.byref(spec),
                                  ctypes.byref(hs) if hs is not None else None, stats.data_ptr(),
                                  counts.data_ptr() if counts is not None else None, stream)
    if rc != 0:
        raise _lib.LnsError("lns_op_field_stats failed (%d): %s" % (rc, L.lns_create_error().decode()))
    return stats, counts


FLOW_STATS = ("ke_P", "ke_Q", "ens_P", "ens_Q", "div_P", "div_Q", "vort_err", "vort_cos", "vel_err", "maxvort_P", "maxvort_Q",
              "maxdiv_P")
FLOW_BOUNDARIES = ("periodic", "wall")


def flow_boundary(boundary, cfg=None):
    """(bc_y, bc_x) as LNS_FLOW_PERIODIC / LNS_FLOW_WALL (0 / 1) from "periodic", "wall", a pair (y, x) of the two names, or
    "auto": per axis "periodic" where the model's autoencoder pads that axis circularly (cfg.ae_pad_y / ae_pad_x of an engine's
    configuration), else "wall" -- the rule of `spectrum_basis`: periodic / periodic for ns2d*, wall / periodic for
    sw_half_periodic, wall / wall for the two-phase presets.  Host only; anything else raises LnsError."""
    def one(b):
        if not isinstance(b, str) or b not in FLOW_BOUNDARIES:
            raise _lib.LnsError('flow boundary: "periodic", "wall", a pair (y, x) of them or "auto", got %r' % (boundary,))
        return FLOW_BOUNDARIES.index(b)
    if isinstance(boundary, str):
        if boundary == "auto":
            if cfg is None:
                raise _lib.LnsError('flow boundary "auto" needs a model (Engine.flow_stats / the rollout calls): '
                                    'name the boundaries of stored fields')
            return tuple(0 if pad == _lib.LNS_PAD_CIRCULAR else 1 for pad in (cfg.ae_pad_y, cfg.ae_pad_x))
        return one(boundary), one(boundary)
    try:
        by, bx = boundary
    except (TypeError, ValueError):
        raise _lib.LnsError('flow boundary: "periodic", "wall", a pair (y, x) of them or "auto", got %r' % (boundary,))
    return one(by), one(bx)


def _flow_fields(name, tensors):
    for t in tensors:
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 5:
            raise _lib.LnsError("%s takes fp32 HIP tensors [B,T,C,H,W] (no CPU fallback)" % name)


def flow_stats(y_hat, y, u=0, v=1, dx=1.0, dy=1.0, boundary="periodic", vort_hist=None, mean=0.0, std=1.0, eps=1e-8,
               zero_wall_channels=(), clamp_channels=(), clamp=(0.0, 1.0 + 1e-8)):
    """Flow diagnostics of stored fields (lns_op_flow_stats; include/lns.h "flow diagnostics"): y_hat and y [B,T,C,H,W],
    normalised, denormalised as in `relative_l2` into forecast P and truth Q; channels u (x-component) and v are the velocity
    pair, dx / dy the grid spacings, `boundary` what `flow_boundary` takes ("auto" needs a model: Engine.flow_stats).
    Returns (flow [B,T,12], hist): the columns are FLOW_STATS -- mean kinetic energy and enstrophy of P and Q, their rms
    divergence, the relative L2 error and the cosine of the vorticity, the relative L2 error of the velocity, and the largest
    |vorticity| of P and Q and |divergence| of P.  Derivatives are central differences, wrapped on a periodic axis and
    one-sided at the two ends of a wall axis (numpy.gradient).  vort_hist = (nbins, lo, hi) adds the int32 counts
    [B,T,2,nbins+2] of the vorticity (rows forecast, truth; bins as `histogram_edges`), else None.
    The kernel body of Engine.rollout_eval_flow."""
    from .engine import eval_spec, flow_spec
    fs = flow_spec(u, v, dx, dy, boundary, vort_hist)                  # (a bad boundary is named before the tensors are looked at)
    _flow_fields("flow_stats", (y_hat, y))
    if y.shape != y_hat.shape or y.device != y_hat.device:
        raise _lib.LnsError("y must have y_hat's shape %s and device, got %s" % (tuple(y_hat.shape), tuple(y.shape)))
    B, T, C, H, W = (int(n) for n in y_hat.shape)
    y_hat, y = y_hat.contiguous(), y.contiguous()
    spec = eval_spec(C, mean=mean, std=std, eps=eps, zero_wall_channels=zero_wall_channels, clamp_channels=clamp_channels,
                     clamp=clamp)
    flow = torch.empty((B, T, _lib.LNS_FLOW_STATS), dtype=torch.float32, device=y_hat.device)
    counts = torch.empty((B, T, 2, fs.nbins + 2), dtype=torch.int32, device=y_hat.device) if fs.nbins else None
    L = _lib.lib()
    with torch.cuda.device(y_hat.device):
        stream = ctypes.c_void_p(torch.cuda.current_stream(y_hat.device).cuda_stream)
        rc = L.lns_op_flow_stats(y_hat.data_ptr(), y.data_ptr(), B, T, C, H, W, ctypes.byref(spec), ctypes.byref(fs),
                                 flow.data_ptr(), counts.data_ptr() if counts is not None else None, stream)
    if rc != 0:
        raise _lib.LnsError("lns_op_flow_stats failed (%d): %s" % (rc, L.lns_create_error().decode()))
    return flow, counts


def vorticity(fields, u=0, v=1, dx=1.0, dy=1.0, boundary="periodic", mean=0.0, std=1.0, eps=1e-8, zero_wall_channels=(),
              clamp_channels=(), clamp=(0.0, 1.0 + 1e-8)):
    """The vorticity dv/dx - du/dy of stored fields (lns_op_vorticity): fields [B,T,C,H,W], normalised (a forecast or the
    truth), denormalised and differenced as in `flow_stats` -> [B,T,H,W].  The pixel function of the statistics and of the
    vort_frames of Engine.rollout_eval_flow."""
    from .engine import eval_spec, flow_spec
    fs = flow_spec(u, v, dx, dy, boundary, None)
    _flow_fields("vorticity", (fields,))
    B, T, C, H, W = (int(n) for n in fields.shape)
    fields = fields.contiguous()
    spec = eval_spec(C, mean=mean, std=std, eps=eps, zero_wall_channels=zero_wall_channels, clamp_channels=clamp_channels,
                     clamp=clamp)
    out = torch.empty((B, T, H, W), dtype=torch.float32, device=fields.device)
    L = _lib.lib()
    with torch.cuda.device(fields.device):
        stream = ctypes.c_void_p(torch.cuda.current_stream(fields.device).cuda_stream)
        rc = L.lns_op_vorticity(fields.data_ptr(), B, T, C, H, W, ctypes.byref(spec), ctypes.byref(fs), out.data_ptr(), stream)
    if rc != 0:
        raise _lib.LnsError("lns_op_vorticity failed (%d): %s" % (rc, L.lns_create_error().decode()))
    return out


def histogram_edges(nbins, lo, hi):
    """The nbins + 1 edges lo + k (hi - lo) / nbins of the interior bins of a field_stats histogram, float64 [nbins + 1]
    (lo, hi scalars) or [C, nbins + 1] (per channel).  Bin 0 of the counts lies below edges[0], bin k in 1 .. nbins between
    edges[k - 1] and edges[k], bin nbins + 1 from edges[-1] on.  (The kernel places a value by (v - lo) * (nbins / (hi - lo))
    in fp32: a value within rounding of an interior edge may fall on either side.)"""
    lo_t = torch.as_tensor(lo, dtype=torch.float64)
    hi_t = torch.as_tensor(hi, dtype=torch.float64)
    k = torch.arange(int(nbins) + 1, dtype=torch.float64) / int(nbins)
    return lo_t.unsqueeze(-1) + (hi_t - lo_t).unsqueeze(-1) * k


def correlation_time(corr, steps, threshold=0.8):
    """corr [B, n, C] (column `corr` or `cos` of field statistics taken at `steps`, n ascending steps) -> int64 [B, C]: the
    first of `steps` at which the correlation is below `threshold`, -1 where it never is (a NaN is not below)."""
    steps_t = torch.as_tensor(list(steps), dtype=torch.int64, device=corr.device)
    if corr.dim() != 3 or corr.shape[1] != steps_t.numel():
        raise _lib.LnsError("correlation_time takes corr [B, n, C] and n steps, got %s and %d" % (tuple(corr.shape), steps_t.numel()))
    below = corr < threshold
    first = below.to(torch.int64).argmax(dim=1)
    return torch.where(below.any(dim=1), steps_t[first], torch.full_like(first, -1))


TIME_MAPS = ("mean_P", "mean_Q", "var_P", "var_Q", "cov", "mse", "max_err")


def time_maps(y_hat, y, map_steps=None, mean=0.0, std=1.0, eps=1e-8, zero_wall_channels=(), clamp_channels=(), clamp=(0.0, 1.0 + 1e-8)):
    """Per-pixel time maps of stored fields (lns_op_time_maps; include/lns.h "time maps"): y_hat and y [B,T,C,H,W], normalised,
    denormalised as in `relative_l2` into forecast P and truth Q.  Returns [B,C,7,H,W], the planes TIME_MAPS: the time-means
    of P and Q, their unbiased temporal variances and covariance, the mean squared error and the largest absolute error, over
    the steps `map_steps` (None: every step; slice(from, None, every) or (from, every)).  Sums are float64, shifted by the
    truth's first frame.  The kernel body of Engine.rollout_eval_maps."""
    from .engine import eval_spec, normalize_map_steps
    first, every = normalize_map_steps(map_steps)
    for t in (y_hat, y):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 5:
            raise _lib.LnsError("time_maps takes fp32 HIP tensors [B,T,C,H,W] (no CPU fallback)")
    if y.shape != y_hat.shape or y.device != y_hat.device:
        raise _lib.LnsError("y must have y_hat's shape %s and device, got %s" % (tuple(y_hat.shape), tuple(y.shape)))
    B, T, C, H, W = (int(v) for v in y_hat.shape)
    y_hat, y = y_hat.contiguous(), y.contiguous()
    spec = eval_spec(C, mean=mean, std=std, eps=eps, zero_wall_channels=zero_wall_channels, clamp_channels=clamp_channels,
                     clamp=clamp)
    L = _lib.lib()
    need = ctypes.c_size_t(0)
    if L.lns_time_maps_state_bytes(B, C, H, W, ctypes.byref(need)) != 0:
        raise _lib.LnsError("lns_time_maps_state_bytes failed: %s" % L.lns_create_error().decode())
    maps = torch.empty((B, C, _lib.LNS_TIME_MAPS, H, W), dtype=torch.float32, device=y_hat.device)
    state = torch.empty(int(need.value), dtype=torch.uint8, device=y_hat.device)
    with torch.cuda.device(y_hat.device):
        stream = ctypes.c_void_p(torch.cuda.current_stream(y_hat.device).cuda_stream)
        rc = L.lns_op_time_maps(y_hat.data_ptr(), y.data_ptr(), B, T, C, H, W, ctypes.byref(spec), first, every, maps.data_ptr(),
                                state.data_ptr(), state.numel(), stream)
    if rc != 0:
        raise _lib.LnsError("lns_op_time_maps failed (%d): %s" % (rc, L.lns_create_error().decode()))
    return maps


def rmse_map(maps):
    """maps [.., 7, H, W] (time_maps, EvalMaps.maps) -> the root mean squared error per pixel, [.., H, W]."""
    return maps[..., TIME_MAPS.index("mse"), :, :].sqrt()


def temporal_correlation(maps):
    """maps [.., 7, H, W] -> cov / sqrt(var_P var_Q) per pixel, [.., H, W]; 0 where either variance is 0 (a pixel constant in
    time, or maps over a single step)."""
    vP, vQ, cov = (maps[..., TIME_MAPS.index(k), :, :] for k in ("var_P", "var_Q", "cov"))
    den = vP.sqrt() * vQ.sqrt()
    return torch.where(den == 0, torch.zeros_like(den), cov / den)


def error_attribution(y_hat, r, y, mean=0.0, std=1.0, eps=1e-8, zero_wall_channels=(), clamp_channels=(), clamp=(0.0, 1.0 + 1e-8)):
    """The rollout error of stored fields split at the reconstruction (lns_op_eval_attrib; include/lns.h "error attribution"):
    y_hat (forecast), r (the autoencoder's reconstruction of the truth) and y [B,T,C,H,W], normalised, denormalised as in
    `relative_l2`.  Returns (prop_frame [B,T,C], prop_seq [B,C], cross_frame, cross_seq): prop = ||y_hat - r|| / ||y||, the
    propagator's error seen through the decoder, and cross = 2 <y_hat - r, r - y> / ||y||^2, so that with
    recon = relative_l2(r, y) and frame = relative_l2(y_hat, y): frame^2 = prop^2 + recon^2 + cross.  The kernel bodies of
    Engine.rollout_eval_attrib."""
    from .engine import eval_spec
    for t in (y_hat, r, y):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 5:
            raise _lib.LnsError("error_attribution takes fp32 HIP tensors [B,T,C,H,W] (no CPU fallback)")
    for t in (y_hat, r):
        if t.shape != y.shape or t.device != y.device:
            raise _lib.LnsError("y_hat and r must have y's shape %s and device, got %s" % (tuple(y.shape), tuple(t.shape)))
    B, T, C, H, W = (int(v) for v in y.shape)
    y_hat, r, y = y_hat.contiguous(), r.contiguous(), y.contiguous()
    spec = eval_spec(C, mean=mean, std=std, eps=eps, zero_wall_channels=zero_wall_channels, clamp_channels=clamp_channels,
                     clamp=clamp)
    out = [torch.empty(s, dtype=torch.float32, device=y.device) for s in ((B, T, C), (B, C), (B, T, C), (B, C))]
    L = _lib.lib()
    with torch.cuda.device(y.device):
        stream = ctypes.c_void_p(torch.cuda.current_stream(y.device).cuda_stream)
        rc = L.lns_op_eval_attrib(y_hat.data_ptr(), r.data_ptr(), y.data_ptr(), B, T, C, H, W, ctypes.byref(spec),
                                  *(t.data_ptr() for t in out), stream)
    if rc != 0:
        raise _lib.LnsError("lns_op_eval_attrib failed (%d): %s" % (rc, L.lns_create_error().decode()))
    return tuple(out)


def attribution_shares(frame, prop, recon, cross):
    """The three shares of frame^2 (columns of Engine.rollout_eval_attrib, frame- or sequence-wise): (prop^2, recon^2, cross)
    / frame^2 -- what the propagator adds, the autoencoder's floor, and their interaction (signed).  They sum to 1 up to
    rounding; NaN where frame is 0.  Host-side helper: plain tensor arithmetic on the small result columns."""
    f2 = frame * frame
    return prop * prop / f2, recon * recon / f2, cross / f2


def spread_skill_ratio(scores, members):
    """spread * sqrt((M + 1) / M) / rmse of an `engine.EnsembleScores` (Engine.rollout_latent_ensemble_eval,
    LatentDynamics.validate_ensemble) with M = `members`: near 1 for a calibrated ensemble, below it for an
    under-dispersive one (the finite-ensemble correction of the spread-skill relation)."""
    members = int(members)
    if members < 2:
        raise ValueError("spread_skill_ratio needs at least 2 members")
    return scores.spread * float((members + 1) / members) ** 0.5 / scores.rmse


def quantile_positions(quantiles, members):
    """[(lo, frac)] of the probabilities among `members` sorted values, as include/lns.h states it: h = p (M - 1) in double,
    lo = floor(h), frac = (float)(h - lo), and lo = M - 1 forces frac = 0."""
    import math
    import numpy as np
    M = int(members)
    out = []
    for p in quantiles:
        p = float(p)
        if not 0.0 <= p <= 1.0:                                   # (a NaN fails both comparisons)
            raise ValueError("a quantile's probability must be in [0, 1], got %r" % (p,))
        h = p * (M - 1)
        lo = int(math.floor(h))
        frac = float(np.float32(h - lo))
        out.append((M - 1, 0.0) if lo >= M - 1 else (lo, frac))
    return out


def threshold_table(thresholds, C):
    """thresholds (each a scalar for every channel, or a per-channel sequence of C values) -> [[float] * C] per threshold."""
    rows = []
    for t in thresholds:
        row = [float(t)] * C if isinstance(t, (int, float)) else [float(v) for v in t]
        if len(row) != C:
            raise ValueError("a per-channel threshold needs %d entries, got %d" % (C, len(row)))
        rows.append(row)
    return rows


def _denormalise(x, mean=0.0, std=1.0, eps=1e-8, zero_wall_channels=(), clamp_channels=(), clamp=(0.0, 1.0 + 1e-8)):
    """D_c of include/lns.h on x [..., C, H, W] in unfused fp32 torch ops: x * std_c + mean_c (the product and the sum rounded on
    their own), 0 on the wall rows / columns of `zero_wall_channels`, fmin(fmax(., lo), hi) on `clamp_channels`."""
    C, H, W = x.shape[-3:]

    def per_c(v):
        v = [float(v)] * C if isinstance(v, (int, float)) else [float(e) for e in v]
        if len(v) != C:
            raise ValueError("per-channel statistics need %d entries" % C)
        return torch.tensor(v, dtype=torch.float32, device=x.device).view(C, 1, 1)
    p = x * per_c(std)
    v = p + per_c(mean)
    if len(zero_wall_channels) > 0:
        mask = torch.zeros((C, H, W), dtype=torch.bool, device=x.device)
        for c in zero_wall_channels:
            mask[c, 0, :] = mask[c, -1, :] = True
            mask[c, :, 0] = mask[c, :, -1] = True
        v = torch.where(mask, torch.zeros_like(v), v)
    if len(clamp_channels) > 0:
        lo = torch.tensor(float(clamp[0]), dtype=torch.float32, device=x.device)
        hi = torch.tensor(float(clamp[1]), dtype=torch.float32, device=x.device)
        sel = torch.zeros((C, 1, 1), dtype=torch.bool, device=x.device)
        for c in clamp_channels:
            sel[c] = True
        v = torch.where(sel.expand(C, H, W), torch.fmin(torch.fmax(v, lo), hi), v)
    return v


def sort_by_bits(v, dim=0):
    """fp32 `v` sorted ascending along `dim` by the total order of the IEEE bit patterns (include/lns.h):
    key(x) = bits ^ (sign ? 0xFFFFFFFF : 0x80000000) compared as unsigned -- held in int64, sorted, and mapped back, so -0 lies
    below +0, NaNs are ordered by their sign, and the result is the same bits whatever the sorting algorithm."""
    bits = v.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    key = bits ^ torch.where(bits >= 0x80000000, torch.full_like(bits, 0xFFFFFFFF), torch.full_like(bits, 0x80000000))
    key = key.sort(dim=dim).values
    bits = key ^ torch.where(key >= 0x80000000, torch.full_like(key, 0x80000000), torch.full_like(key, 0xFFFFFFFF))
    bits = torch.where(bits >= 0x80000000, bits - 0x100000000, bits)
    return bits.to(torch.int32).view(torch.float32)


@torch.no_grad()
def ensemble_quantiles(fields, quantiles=(), thresholds=(), **norm):
    """The stored-path statement of Engine.rollout_latent_ensemble_quantiles / ensemble_quantiles (include/lns.h "ensemble
    quantiles") in unfused fp32 torch ops, on whatever device `fields` lives on: fields [B, M, n, C, H, W], the stored member
    rollouts -> (quantiles [B, n, n_q, C, H, W] or None, prob [B, n, n_thr, C, H, W] or None).  `norm` as in `relative_l2`
    (none: the values as they are).  It needs the member fields the streaming call never stores: for checks and small cases."""
    if fields.dim() != 6 or fields.dtype != torch.float32:
        raise ValueError("expected fp32 member fields [B, M, n, C, H, W]")
    B, M, n, C, H, W = fields.shape
    pos = quantile_positions(quantiles, M)
    thr = threshold_table(thresholds, C)
    if not pos and not thr:
        raise ValueError("neither a quantile nor a threshold was asked for")
    v = _denormalise(fields, **norm) if norm else fields
    v = sort_by_bits(v.permute(1, 0, 2, 3, 4, 5), dim=0)                 # [M, B, n, C, H, W]
    quant = prob = None
    if pos:
        rows = []
        for lo, frac in pos:
            if frac == 0.0:
                rows.append(v[lo])
                continue
            d = v[lo + 1] - v[lo]
            t = torch.full_like(d, frac) * d
            rows.append(v[lo] + t)
        quant = torch.stack(rows, 2)
    if thr:
        fm = torch.full((B, n, C, H, W), float(M), dtype=torch.float32, device=fields.device)
        rows = []
        for row in thr:
            th = torch.tensor(row, dtype=torch.float32, device=fields.device).view(C, 1, 1)
            rows.append((v > th).sum(0).to(torch.float32) / fm)
        prob = torch.stack(rows, 2)
    return quant, prob


@torch.no_grad()
def exceedance_table(fields, y, thresholds, **norm):
    """The stored-path statement of Engine.rollout_latent_ensemble_exceed / ensemble_exceed (include/lns.h "ensemble
    exceedance") in elementwise torch ops and `bincount`, on whatever device `fields` lives on: fields [B, M, n, C, H, W], the
    stored member rollouts, y [B, n, C, H, W] the truth of the same steps -> int32 table [B, n, n_thr, C, 2, M + 1]: per plane
    and threshold the number of pixels with the truth above the threshold (dim 4: 1) or not (0) and n members above it
    (dim 5).  `norm` as in `relative_l2` (none: the values as they are).  It needs the member fields the streaming call never
    stores: for checks and small cases."""
    if fields.dim() != 6 or fields.dtype != torch.float32:
        raise ValueError("expected fp32 member fields [B, M, n, C, H, W]")
    B, M, n, C, H, W = fields.shape
    if tuple(y.shape) != (B, n, C, H, W) or y.dtype != torch.float32 or y.device != fields.device:
        raise ValueError("expected the fp32 truth [B, n, C, H, W] of the member fields, on their device")
    thr = threshold_table(thresholds, C)
    if not 1 <= len(thr) <= 8:
        raise ValueError("between 1 and 8 thresholds per call, got %d" % len(thr))
    v = _denormalise(fields, **norm) if norm else fields
    q = _denormalise(y, **norm) if norm else y
    M1 = M + 1
    plane = torch.arange(B * n * C, dtype=torch.int64, device=fields.device).view(B, n, C, 1, 1) * (2 * M1)
    rows = []
    for row in thr:
        th = torch.tensor(row, dtype=torch.float32, device=fields.device).view(C, 1, 1)
        cnt = (v > th).sum(1, dtype=torch.int64)                        # [B, n, C, H, W]: n of the statement
        obs = (q > th).to(torch.int64)
        idx = plane + obs * M1 + cnt
        rows.append(torch.bincount(idx.reshape(-1), minlength=B * n * C * 2 * M1).view(B, n, C, 2, M1))
    return torch.stack(rows, 2).to(torch.int32)


def _table64(table):
    """An exceedance table [..., 2, M + 1] (torch or numpy, any integer type) -> (N0, N1, M) as float64 numpy arrays [..., M + 1]."""
    import numpy as np
    t = table.detach().cpu().numpy() if isinstance(table, torch.Tensor) else np.asarray(table)
    if t.ndim < 2 or t.shape[-2] != 2 or t.shape[-1] < 2:
        raise ValueError("expected an exceedance table [..., 2, M + 1], got %s" % (tuple(t.shape),))
    t = t.astype(np.float64)
    return t[..., 0, :], t[..., 1, :], t.shape[-1] - 1


BrierScores = collections.namedtuple("BrierScores", "bs bs_fair reliability resolution uncertainty base_rate")
BrierScores.__doc__ = """metrics.brier_scores: the Brier score, its fair (member-count corrected) form, the reliability,
resolution and uncertainty terms (bs = reliability - resolution + uncertainty) and the event's base rate; float64 [...]."""
RocCurve = collections.namedtuple("RocCurve", "pofd pod auc")
RocCurve.__doc__ = """metrics.roc_curve: probability of false detection and of detection [..., M + 2] for the cut-offs n >= j,
j = M + 1 .. 0 (from (0, 0) to (1, 1)), and the area under them by the trapezoid rule [...]; float64."""
ContingencyScores = collections.namedtuple("ContingencyScores", "hits misses false_alarms correct_negatives pod far csi")
ContingencyScores.__doc__ = """metrics.contingency_scores: the 2 x 2 counts (int64 [...]) of the forecast "at least min_members
members above the threshold" and POD = hits / (hits + misses), FAR = false_alarms / (hits + false_alarms), CSI = hits /
(hits + misses + false_alarms) -- the IoU of the forecast region and the true one; float64 [...], NaN over 0."""


def brier_scores(table):
    """Brier score of the exceedance probability p = n / M and its decomposition, from an exceedance table [..., 2, M + 1]
    (frame-wise as the call returns it, or `table.sum(1, dtype=torch.int64)` for the sequence-wise form); float64, on the host.
    With N[o][n] the counts, N their sum, p_n = n / M, N_n = N[0][n] + N[1][n], obar_n = N[1][n] / N_n (empty bins skipped),
    base = sum N[1] / N:
        bs = (1/N) sum_n [N[1][n] (1 - p_n)^2 + N[0][n] p_n^2]
        reliability = (1/N) sum N_n (p_n - obar_n)^2;  resolution = (1/N) sum N_n (obar_n - base)^2;  uncertainty = base (1 - base)
        bs_fair = bs - (1/N) sum N_n n (M - n) / (M^2 (M - 1))          (M = 1: bs_fair = bs)
    The forecast takes M + 1 values only, so bs = reliability - resolution + uncertainty exactly (no within-bin term).  An
    event that never or always occurs has uncertainty = resolution = 0 and bs = reliability; members that all agree have
    bs_fair = bs; an empty table (N = 0) gives NaN."""
    import numpy as np
    N0, N1, M = _table64(table)
    n = np.arange(M + 1, dtype=np.float64)
    p = n / M
    Nn = N0 + N1
    with np.errstate(divide="ignore", invalid="ignore"):
        N = Nn.sum(-1)
        inv = np.where(N > 0, 1.0 / N, np.nan)
        base = N1.sum(-1) * inv
        obar = np.where(Nn > 0, N1 / np.where(Nn > 0, Nn, 1.0), 0.0)
        bs = (N1 * (1.0 - p) ** 2 + N0 * p ** 2).sum(-1) * inv
        rel = (Nn * (p - obar) ** 2).sum(-1) * inv                      # (an empty bin has N_n = 0: no term)
        res = (Nn * (obar - base[..., None]) ** 2).sum(-1) * inv
        unc = base * (1.0 - base)
        fair = bs - (Nn * (n * (M - n) / (M * M * (M - 1.0)))).sum(-1) * inv if M > 1 else bs.copy()
    return BrierScores(bs, fair, rel, res, unc, base)


def reliability_curve(table):
    """The reliability diagram of an exceedance table [..., 2, M + 1]: (p_n [M + 1], obar_n [..., M + 1], N_n [..., M + 1]) --
    the forecast probability n / M, the observed frequency of the event among the pixels that got it (NaN for an empty bin)
    and their number (int64); float64, on the host."""
    import numpy as np
    N0, N1, M = _table64(table)
    Nn = N0 + N1
    with np.errstate(divide="ignore", invalid="ignore"):
        obar = np.where(Nn > 0, N1 / np.where(Nn > 0, Nn, 1.0), np.nan)
    return np.arange(M + 1, dtype=np.float64) / M, obar, Nn.astype(np.int64)


def roc_curve(table):
    """The ROC curve of an exceedance table [..., 2, M + 1]: the forecast "at least j members above the threshold" for
    j = M + 1 .. 0 has pod_j = sum_{n >= j} N[1][n] / sum N[1] and pofd_j = sum_{n >= j} N[0][n] / sum N[0] (M + 2 points from
    (0, 0) to (1, 1)); auc by the trapezoid rule, which is the Mann-Whitney statistic P(n_event > n_other) + P(equal) / 2.
    Where the event never occurs pod and auc are NaN, where it always occurs pofd and auc are NaN.  RocCurve, float64."""
    import numpy as np
    N0, N1, M = _table64(table)

    def tail(Nx):                                                       # j = M + 1 .. 0: 0, N[M], N[M] + N[M-1], ...
        c = np.cumsum(Nx[..., ::-1], -1)
        c = np.concatenate([np.zeros_like(c[..., :1]), c], -1)
        tot = c[..., -1:]
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(tot > 0, c / np.where(tot > 0, tot, 1.0), np.nan)
    pofd, pod = tail(N0), tail(N1)
    auc = ((pofd[..., 1:] - pofd[..., :-1]) * (pod[..., 1:] + pod[..., :-1]) * 0.5).sum(-1)
    return RocCurve(pofd, pod, auc)


def contingency_scores(table, min_members):
    """Hits, misses, false alarms and correct negatives of the yes / no forecast "at least `min_members` of the M members
    above the threshold" (1 <= min_members <= M) from an exceedance table [..., 2, M + 1], and POD, FAR, CSI from them
    (ContingencyScores).  With M = 1 and min_members = 1 this is the deterministic forecast's table, and CSI the IoU of the
    forecast region and the true one.  A ratio over 0 (no event and no forecast of it) is NaN."""
    import numpy as np
    N0, N1, M = _table64(table)
    j = int(min_members)
    if not 1 <= j <= M:
        raise ValueError("min_members must be in 1 .. %d, got %d" % (M, j))
    hits, misses = N1[..., j:].sum(-1), N1[..., :j].sum(-1)
    fa, cn = N0[..., j:].sum(-1), N0[..., :j].sum(-1)

    def ratio(a, b):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(b > 0, a / np.where(b > 0, b, 1.0), np.nan)
    i64 = lambda a: a.astype(np.int64)                                  # noqa: E731
    return ContingencyScores(i64(hits), i64(misses), i64(fa), i64(cn), ratio(hits, hits + misses), ratio(fa, hits + fa),
                             ratio(hits, hits + misses + fa))


def sw_norm(u_mean, u_std, v_mean, v_std, pres_mean, pres_std):
    """Keyword arguments for encode_dataset restating Stage2_SW.normalize (dataset/Stage2_SW.py:74-78): channels
    (u, v, pres), each by its own statistics, no epsilon."""
    return dict(mean=[u_mean, v_mean, pres_mean], std=[u_std, v_std, pres_std], eps=0.0)


def twophase_norm(vel_mean, vel_std, prs_mean, prs_std):
    """Keyword arguments for encode_dataset restating TwoPhaseFlow.normalize_data + the channel layout of its
    encode_dataset (dataset/twophase_flow_stage2.py:304-313, :325-326): (u, v) by the velocity statistics, pressure by its
    own, the VOF channel as is; chunks of 32 frames (:329-334)."""
    return dict(mean=[vel_mean, vel_mean, prs_mean, 0.0], std=[vel_std, vel_std, prs_std, 1.0], eps=0.0, chunk=32)


@torch.no_grad()
def encode_dataset(autoencoder, frames, chunk=32, mean=0.0, std=1.0, eps=1e-8, out_device="cpu", param=None):
    """Pre-encodes a whole trajectory set for stage-2 training: frames [N,C,H,W] (raw, un-normalised; torch tensor or
    numpy array) -> latents [N, latent_dim, h, w], `chunk` frames per encoder call, with the dataset normalisation
    (u - mean) / (std + eps) applied first on the device.  mean / std: scalars (NS2d,
    dataset/ns2d_fno_stage2_simpleae.py:78-93) or per-channel sequences (`sw_norm(...)`: dataset/Stage2_SW.py:74-105;
    `twophase_norm(...)`: dataset/twophase_flow_stage2.py:304-337).  `param` [N] (one value per frame) is passed to a
    ConditionalSimpleAutoencoder's encode."""
    frames = torch.as_tensor(frames)
    dev = next(iter(autoencoder.parameters())).device
    C = frames.shape[1]

    def stat(v):
        v = [float(v)] * C if isinstance(v, (int, float)) else [float(e) for e in v]
        if len(v) != C:
            raise ValueError("per-channel statistics need %d entries" % C)
        return v
    # (u - mean) / (std + eps) = u * scale + shift, in fp64 on the host: 2 C numbers.  The map is applied inside the
    # encoder's first convolution (its per-(sample, channel) scale / shift prologue, lns_encode_affine): no normalised copy
    # of the frames is ever written, and no tensor arithmetic runs outside the HIP kernels.
    m, sd = stat(mean), stat(std)
    table = torch.tensor([[1.0 / (s_ + eps), -m_ / (s_ + eps)] for m_, s_ in zip(m, sd)], dtype=torch.float64)
    table = table.to(torch.float32).to(dev)
    if param is not None:
        param = torch.as_tensor(param)
    outs = []
    for s in range(0, frames.shape[0], chunk):
        u = frames[s:s + chunk].to(dev, dtype=torch.float32)
        ss = table.unsqueeze(0).expand(u.shape[0], C, 2).contiguous()
        eng = autoencoder._engine(u)
        z = eng.encode(u, None if param is None else param[s:s + chunk].to(dev), scale_shift=ss)
        outs.append(z.to(out_device))
    return torch.cat(outs, 0)

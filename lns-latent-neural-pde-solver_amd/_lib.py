"""ctypes binding of liblns_hip.so (the C ABI of include/lns.h).

There is NO fallback: if the HIP library is missing the import of any compute
path fails loudly (LnsLibraryError).  `build()` compiles it in-tree with hipcc
for gfx950 (cross-compiles without a GPU).
"""
import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
# LNS_HIP_LIB: A/B runs of two builds of the library inside one GPU call (tools/ab_bench.sh); never set in production
LIB_PATH = os.environ.get("LNS_HIP_LIB") or os.path.join(_HERE, "liblns_hip.so")
CSRC = os.path.join(_HERE, "csrc")

LNS_MAX_STAGES = 8
LNS_ABI_VERSION = 2
LNS_AE_NONE, LNS_AE_SQUARE, LNS_AE_NONSQUARED, LNS_AE_HALF_PERIODIC = 0, 1, 2, 3
LNS_PROP_NONE, LNS_PROP_PLAIN, LNS_PROP_CONDITIONAL = 0, 1, 2
LNS_PAD_ZEROS, LNS_PAD_CIRCULAR = 0, 1
LNS_SPECTRUM_DFT, LNS_SPECTRUM_DCT = 0, 1
# status codes (include/lns.h)
LNS_OK, LNS_EINVAL, LNS_ENOKEY, LNS_ESTATE, LNS_ENOMEM, LNS_EHIP, LNS_ENONFINITE = 0, -1, -2, -3, -4, -5, -6


class LnsLibraryError(RuntimeError):
    pass


class LnsError(RuntimeError):
    pass


_I32 = ctypes.c_int32
_I32x8 = ctypes.c_int32 * LNS_MAX_STAGES


class LnsConfig(ctypes.Structure):
    """Mirror of `struct lns_config` (include/lns.h)."""
    _fields_ = [
        ("abi_version", _I32), ("ae_kind", _I32), ("prop_kind", _I32),
        ("in_channels", _I32), ("latent_dim", _I32), ("Ly", _I32), ("Lx", _I32),
        ("res_h", _I32), ("res_w", _I32), ("latent_resolution", _I32),
        ("ae_pad_y", _I32), ("ae_pad_x", _I32),
        ("n_encoder_channels", _I32), ("encoder_channels", _I32x8),
        ("encoder_res_blocks", _I32), ("use_attn_enc", _I32),
        ("n_decoder_channels", _I32), ("decoder_channels", _I32x8),
        ("decoder_res_blocks", _I32),
        ("n_attn_resolutions", _I32), ("attn_resolutions", _I32x8),
        ("n_fourier_resolutions", _I32), ("fourier_resolutions", _I32x8),
        ("use_fa", _I32), ("final_smoothing", _I32), ("disable_coarse_attn", _I32),
        ("attn_heads", _I32), ("attn_dim", _I32),
        ("hw_ratio", ctypes.c_float),
        ("prop_n_block", _I32), ("prop_n_embd", _I32), ("prop_dilation", _I32),
        ("prop_pad_y", _I32), ("prop_pad_x", _I32), ("cond_emb_dim", _I32),
        ("ae_prefix", ctypes.c_char * 32), ("prop_prefix", ctypes.c_char * 32),
        ("cond_encoder", _I32), ("cond_emb_channels", _I32),
    ]


LNS_METRIC_MAX_CH = 8
_F32x8 = ctypes.c_float * LNS_METRIC_MAX_CH


class LnsEvalSpec(ctypes.Structure):
    """Mirror of `struct lns_eval_spec` (include/lns.h): the denormalisation of the streaming evaluation."""
    _fields_ = [
        ("size", ctypes.c_uint32), ("per_channel", _I32),
        ("mean", ctypes.c_float), ("std", ctypes.c_float), ("eps", ctypes.c_float),
        ("mean_c", _F32x8), ("std_c", _F32x8), ("flags_c", ctypes.c_int32 * LNS_METRIC_MAX_CH),
        ("clamp_lo", ctypes.c_float), ("clamp_hi", ctypes.c_float),
    ]


class LnsEnsembleQuantileSpec(ctypes.Structure):
    """Mirror of `struct lns_ensemble_quantile_spec` (include/lns.h): the probabilities and thresholds of the ensemble quantiles."""
    _fields_ = [
        ("size", ctypes.c_uint32), ("n_q", _I32), ("n_thr", _I32), ("reserved", ctypes.c_uint32),
        ("q", ctypes.c_double * 8), ("thr", (ctypes.c_float * LNS_METRIC_MAX_CH) * 8),
    ]


class LnsEnsembleExceedSpec(ctypes.Structure):
    """Mirror of `struct lns_ensemble_exceed_spec` (include/lns.h): the thresholds of the exceedance contingency tables."""
    _fields_ = [
        ("size", ctypes.c_uint32), ("n_thr", _I32), ("thr", (ctypes.c_float * LNS_METRIC_MAX_CH) * 8),
    ]


LNS_FIELD_STATS = 12


class LnsStatsSpec(ctypes.Structure):
    """Mirror of `struct lns_stats_spec` (include/lns.h): the value histograms of the field statistics."""
    _fields_ = [("size", ctypes.c_uint32), ("nbins", _I32), ("lo", _F32x8), ("hi", _F32x8)]


LNS_TIME_MAPS = 7


class LnsEvalSelect(ctypes.Structure):
    """Mirror of `struct lns_eval_select` (include/lns.h): the optional selections and outputs of lns_rollout_eval_maps."""
    _fields_ = [
        ("size", ctypes.c_uint32), ("n_spec", _I32), ("n_stats", _I32), ("map_from", _I32), ("map_every", _I32),
        ("reserved", _I32),
        ("spectrum_steps_host", ctypes.POINTER(ctypes.c_int)), ("spectra_out", ctypes.c_void_p),
        ("stats_steps_host", ctypes.POINTER(ctypes.c_int)), ("hspec", ctypes.POINTER(LnsStatsSpec)),
        ("stats_out", ctypes.c_void_p), ("hist_out", ctypes.c_void_p), ("maps_out", ctypes.c_void_p),
    ]


class LnsEvalAttrib(ctypes.Structure):
    """Mirror of `struct lns_eval_attrib` (include/lns.h): the outputs of the error attribution, every pointer nullable."""
    OUTPUTS = ("recon_frame", "recon_seq", "prop_frame", "prop_seq", "cross_frame", "cross_seq", "latent_frame", "latent_seq",
               "z_true_out", "recon_frames_out")
    _fields_ = [("size", ctypes.c_uint32)] + [(n, ctypes.c_void_p) for n in OUTPUTS]


LNS_FLOW_STATS = 12


class LnsFlowSpec(ctypes.Structure):
    """Mirror of `struct lns_flow_spec` (include/lns.h): the velocity channels, boundaries, spacings and vorticity histogram of
    the flow diagnostics."""
    _fields_ = [
        ("size", ctypes.c_uint32), ("cu", _I32), ("cv", _I32), ("bc_y", _I32), ("bc_x", _I32),
        ("dy", ctypes.c_float), ("dx", ctypes.c_float), ("nbins", _I32), ("lo", ctypes.c_float), ("hi", ctypes.c_float),
    ]


class LnsEvalFlow(ctypes.Structure):
    """Mirror of `struct lns_eval_flow` (include/lns.h): the selection and the outputs of lns_rollout_eval_flow."""
    _fields_ = [
        ("size", ctypes.c_uint32), ("n_flow", _I32),
        ("flow_steps_host", ctypes.POINTER(ctypes.c_int)), ("fspec", ctypes.POINTER(LnsFlowSpec)),
        ("flow_out", ctypes.c_void_p), ("hist_out", ctypes.c_void_p), ("vort_frames_out", ctypes.c_void_p),
    ]


LNS_SL1_CHUNK = 4096


class LnsAdamSpec(ctypes.Structure):
    """Mirror of `struct lns_adam_spec` (include/lns.h): torch.optim.Adam's hyper-parameters and the 1-based step count."""
    _fields_ = [
        ("size", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("lr", ctypes.c_double), ("beta1", ctypes.c_double),
        ("beta2", ctypes.c_double), ("eps", ctypes.c_double), ("weight_decay", ctypes.c_double), ("step", ctypes.c_int64),
    ]


LNS_NORM_CHUNK = 2048
LNS_UPDATE_DECOUPLED_WD, LNS_UPDATE_SKIP_NONFINITE = 1, 2


class LnsUpdateSpec(ctypes.Structure):
    """Mirror of `struct lns_update_spec` (include/lns.h): lns_adam_spec's fields, flags (LNS_UPDATE_*) and max_norm."""
    _fields_ = [
        ("size", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("lr", ctypes.c_double), ("beta1", ctypes.c_double),
        ("beta2", ctypes.c_double), ("eps", ctypes.c_double), ("weight_decay", ctypes.c_double), ("step", ctypes.c_int64),
        ("max_norm", ctypes.c_double),
    ]


LNS_OBS_MAX = 64
LNS_FIT_STATE, LNS_FIT_PARAM = 1, 2
LNS_TANGENT_MAX = 32
LNS_GN_CG_MAX = 64


class LnsFitSpec(ctypes.Structure):
    """Mirror of `struct lns_fit_spec` (include/lns.h): what is fitted, the observation table (host arrays), the weight of
    the background term and one lns_update_spec each for the state and for `param`."""
    _fields_ = [
        ("size", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("n_obs", ctypes.c_int32), ("reserved", ctypes.c_int32),
        ("obs_steps", ctypes.POINTER(ctypes.c_int)), ("obs_weight", ctypes.POINTER(ctypes.c_double)),
        ("background", ctypes.c_double), ("state", LnsUpdateSpec), ("param", LnsUpdateSpec),
    ]


class LnsGnSpec(ctypes.Structure):
    """Mirror of `struct lns_gn_spec` (include/lns.h): the observation table (host arrays), the CG step count, the weight
    of the background term, the Levenberg damping and the relative residual at which a sample's CG stops."""
    _fields_ = [
        ("size", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("n_obs", ctypes.c_int32), ("n_cg", ctypes.c_int32),
        ("obs_steps", ctypes.POINTER(ctypes.c_int)), ("obs_weight", ctypes.POINTER(ctypes.c_double)),
        ("background", ctypes.c_double), ("damping", ctypes.c_double), ("cg_tol", ctypes.c_double),
    ]


def _fields(spec):
    """"x:p B:i eps:f ..." -> ctypes fields (p pointer, i int, f float, q int64)."""
    kinds = {"p": ctypes.c_void_p, "i": ctypes.c_int, "f": ctypes.c_float, "q": ctypes.c_int64}
    return [(n, kinds[k]) for n, k in (t.split(":") for t in spec.split())]


class LnsConvGnArgs(ctypes.Structure):
    """Mirror of `struct lns_conv_gn_args` (include/lns.h): the arguments of lns_op_conv_gn."""
    _fields_ = _fields(
        "x:p B:i Cin:i Hin:i Win:i Hv:i Wv:i w_host:p bias_host:p Cout:i ksize:i stride:i dilation:i pad_t:i pad_b:i pad_l:i "
        "pad_r:i mode_y:i mode_x:i ss:p act_in:i act_out:i residual:p badd:p y:p tile_variant:i part_out:p part_in:p geom:p "
        "groups:i eps:f gamma_host:p beta_host:p premul:p ss_out:p w2_host:p bias2_host:p Cout2:i ksize2:i "
        "act_in2:i variant2:i y2:p")


class LnsFaFusedArgs(ctypes.Structure):
    """Mirror of `struct lns_fa_fused_args` (include/lns.h): the arguments of lns_op_fa_fused."""
    _fields_ = _fields(
        "x:p x_bs:q ss:p bound:f w_host:p kx:p ky:p B:i heads:i dim_head:i Cin:i H:i W:i eps:f instnorm:i form:i gpb:i "
        "b_rev:i out:p amax_out:p")


class LnsFaReducerArgs(ctypes.Structure):
    """Mirror of `struct lns_fa_reducer_args` (include/lns.h): the arguments of lns_op_fa_reducer."""
    _fields_ = _fields(
        "mx:p my:p B:i nx:i ny:i C:i Hid:i Out:i form:i to_in_x:p ln_g_x:p ln_b_x:p w1_x:p w2_x:p b2_x:p "
        "to_in_y:p ln_g_y:p ln_b_y:p w1_y:p w2_y:p b2_y:p ux:p uy:p amax_x:p amax_y:p")


class LnsFaLrkArgs(ctypes.Structure):
    """Mirror of `struct lns_fa_lrk_args` (include/lns.h): the arguments of lns_op_fa_lrk."""
    _fields_ = _fields(
        "qk_x:p qk_y:p B_x:i heads_x:i DK_x:i nx:i B_y:i heads_y:i DK_y:i ny:i form:i inv_freq_x:p inv_freq_y:p kx:p ky:p")


# every symbol include/lns.h declares (tests check the library exports them all)
SYMBOLS = [
    "lns_create_error", "lns_create", "lns_destroy", "lns_last_error", "lns_num_params",
    "lns_param_info", "lns_set_weight", "lns_finalize_weights", "lns_latent_shape", "lns_prepare",
    "lns_encode", "lns_encode_cond", "lns_encode_affine", "lns_decode", "lns_propagate", "lns_rollout", "lns_rollout_latent", "lns_check_finite", "lns_set_option",
    "lns_rollout_eval_workspace_bytes", "lns_rollout_eval", "lns_rollout_latent_eval",
    "lns_rollout_select_workspace_bytes", "lns_rollout_select", "lns_rollout_latent_select",
    "lns_rollout_ensemble_workspace_bytes", "lns_rollout_latent_ensemble", "lns_op_ensemble_stats",
    "lns_rollout_latent_ensemble_eval", "lns_op_ensemble_score",
    "lns_rollout_latent_ensemble_quantiles", "lns_op_ensemble_quantiles",
    "lns_rollout_latent_ensemble_exceed", "lns_op_ensemble_exceed",
    "lns_rollout_ensemble_analysis_workspace_bytes", "lns_rollout_latent_ensemble_analysis",
    "lns_op_ensemble_obs_gram", "lns_op_etkf_transform", "lns_op_ensemble_transform",
    "lns_rollout_ensemble_analysis_local_workspace_bytes", "lns_rollout_latent_ensemble_analysis_local",
    "lns_op_ensemble_patch_gram", "lns_op_letkf_combine", "lns_op_ensemble_transform_local",
    "lns_spectrum_bins", "lns_rollout_eval_spectrum", "lns_rollout_latent_eval_spectrum", "lns_op_energy_spectrum",
    "lns_spectrum_bins_basis", "lns_op_energy_spectrum_basis",
    "lns_rollout_eval_stats", "lns_rollout_latent_eval_stats", "lns_op_field_stats",
    "lns_rollout_eval_maps_workspace_bytes", "lns_rollout_eval_maps", "lns_rollout_latent_eval_maps",
    "lns_time_maps_state_bytes", "lns_op_time_maps",
    "lns_rollout_eval_attrib_workspace_bytes", "lns_rollout_eval_attrib", "lns_rollout_latent_eval_attrib",
    "lns_autoencode_eval_workspace_bytes", "lns_autoencode_eval", "lns_op_eval_attrib", "lns_op_latent_err",
    "lns_rollout_eval_flow", "lns_rollout_latent_eval_flow", "lns_op_flow_stats", "lns_op_vorticity",
    "lns_train_workspace_bytes", "lns_train_forward", "lns_train_backward",
    "lns_loss_smooth_l1", "lns_adam_step", "lns_adam_step_tensors", "lns_train_step_workspace_bytes", "lns_train_step",
    "lns_grad_norm_scratch_bytes", "lns_grad_norm_tensors", "lns_grad_scale_tensors", "lns_update_step_tensors",
    "lns_train_step_clip_workspace_bytes", "lns_train_step_clip",
    "lns_train_backward_ex", "lns_loss_obs_mse_scratch_bytes", "lns_loss_obs_mse", "lns_fit_step_workspace_bytes", "lns_fit_step",
    "lns_train_tangent_workspace_bytes", "lns_train_tangent", "lns_op_orthonormalize",
    "lns_train_gn_product_workspace_bytes", "lns_train_gn_product", "lns_op_cg_start", "lns_op_cg_update",
    "lns_fit_gn_step_workspace_bytes", "lns_fit_gn_step",
    "lns_trace_enable", "lns_trace_count", "lns_trace_info", "lns_trace_copy",
    "lns_timing_enable", "lns_timing_count", "lns_timing_info", "lns_timing_mfma_flops", "lns_build_has",
    "lns_op_conv_wgrad_scratch_bytes", "lns_op_conv_wgrad",
    "lns_op_groupnorm_train", "lns_op_gelu_grad", "lns_op_bias_grad",
    "lns_op_fa_reducer", "lns_fa_reducer_fits", "lns_op_fa_lrk", "lns_fa_lrk_fits", "lns_rotary_table", "lns_op_ln_pe", "lns_op_apply",
    "lns_op_conv2d", "lns_op_conv_gn", "lns_op_fa_fused", "lns_op_conv_pair_stress", "lns_op_groupnorm_stats", "lns_op_attention", "lns_op_fa_sandwich", "lns_op_fa_pool", "lns_op_fourier_block",
    "lns_fourier_block_create", "lns_fourier_block_forward", "lns_fourier_block_destroy", "lns_metric_rel_l2", "lns_metric_rel_l2_ch",
]

_lib = None


def build(force=False):
    """Compile liblns_hip.so in-tree (hipcc --offload-arch=gfx950)."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC)
            if f.endswith((".hip", ".cpp", ".h", ".inc"))] + [os.path.join(_HERE, "..", "include", "lns.h")]
    if (not force and os.path.exists(LIB_PATH)
            and all(os.path.getmtime(LIB_PATH) >= os.path.getmtime(s) for s in srcs)):
        return LIB_PATH
    subprocess.check_call(["make", "-s", "-j4", "-C", CSRC])
    return LIB_PATH


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LnsLibraryError(
            "HIP extension %s is missing; run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(there is no CPU fallback for the LNS hot path)" % LIB_PATH)
    try:
        L = ctypes.CDLL(LIB_PATH)
    except OSError as e:
        raise LnsLibraryError("cannot load %s: %s" % (LIB_PATH, e))
    c = ctypes
    vp, i, i64p, fp = c.c_void_p, c.c_int, c.POINTER(c.c_int64), c.POINTER(c.c_float)
    if os.environ.get("LNS_HIP_LIB"):
        # same-box A/B against an EARLIER round's build (tools/ab_*.sh; never set in production): entry points that build
        # does not export yet become stubs that fail when called, so the core path (rollout, timing, op tests) still binds
        def _absent(*_a, **_k):
            raise LnsLibraryError("entry point missing from the library selected by LNS_HIP_LIB")
        for sym in SYMBOLS:
            if not hasattr(L, sym):
                setattr(L, sym, type("Stub", (), {"__call__": staticmethod(_absent), "argtypes": None, "restype": None})())
    L.lns_create_error.restype = c.c_char_p
    L.lns_create.argtypes = [c.POINTER(LnsConfig), c.POINTER(vp)]
    L.lns_destroy.argtypes = [vp]
    L.lns_destroy.restype = None
    L.lns_last_error.argtypes = [vp]
    L.lns_last_error.restype = c.c_char_p
    L.lns_num_params.argtypes = [vp]
    L.lns_param_info.argtypes = [vp, i, c.c_char_p, i, i64p, c.POINTER(i), c.POINTER(i)]
    L.lns_set_weight.argtypes = [vp, c.c_char_p, vp, i64p, i]
    L.lns_finalize_weights.argtypes = [vp, i]
    L.lns_latent_shape.argtypes = [vp, c.POINTER(i), c.POINTER(i), c.POINTER(i)]
    L.lns_prepare.argtypes = [vp, i, c.POINTER(c.c_size_t)]
    L.lns_encode.argtypes = [vp, vp, i, vp, vp, c.c_size_t, vp]
    L.lns_decode.argtypes = [vp, vp, i, vp, vp, c.c_size_t, vp]
    if hasattr(L, "lns_encode_cond"):
        L.lns_encode_cond.argtypes = [vp, vp, vp, i, vp, vp, c.c_size_t, vp]
    L.lns_encode_affine.argtypes = [vp, vp, vp, vp, i, vp, vp, c.c_size_t, vp]
    L.lns_propagate.argtypes = [vp, vp, vp, i, i, i, vp, vp, c.c_size_t, vp]
    L.lns_rollout.argtypes = [vp, vp, vp, i, i, i, vp, vp, vp, c.c_size_t, vp]
    L.lns_rollout_latent.argtypes = [vp, vp, vp, i, i, i, vp, vp, vp, c.c_size_t, vp]
    if hasattr(L, "lns_rollout_eval"):
        sp, ip = c.POINTER(LnsEvalSpec), c.POINTER(c.c_int)
        L.lns_rollout_eval_workspace_bytes.argtypes = [vp, i, c.POINTER(c.c_size_t)]
        L.lns_rollout_eval.argtypes = [vp, vp, vp, vp, i, i, sp, vp, vp, ip, i, vp, vp, c.c_size_t, vp]
        L.lns_rollout_latent_eval.argtypes = [vp, vp, vp, vp, i, i, i, i, sp, vp, vp, ip, i, vp, vp, vp, c.c_size_t, vp]
    if hasattr(L, "lns_rollout_select"):
        ip = c.POINTER(c.c_int)
        L.lns_rollout_select_workspace_bytes.argtypes = [vp, i, c.POINTER(c.c_size_t)]
        L.lns_rollout_select.argtypes = [vp, vp, vp, i, i, ip, i, vp, vp, vp, c.c_size_t, vp]
        L.lns_rollout_latent_select.argtypes = [vp, vp, vp, i, i, ip, i, vp, vp, vp, c.c_size_t, vp]
    if hasattr(L, "lns_rollout_latent_ensemble"):
        ip = c.POINTER(c.c_int)
        L.lns_rollout_ensemble_workspace_bytes.argtypes = [vp, i, i, c.POINTER(c.c_size_t)]
        L.lns_rollout_latent_ensemble.argtypes = [vp, vp, vp, i, i, i, ip, i, vp, vp, vp, vp, c.c_size_t, vp]
        L.lns_op_ensemble_stats.argtypes = [vp, i, i, c.c_int64, vp, vp, vp]
    if hasattr(L, "lns_rollout_latent_ensemble_eval"):
        sp, ip = c.POINTER(LnsEvalSpec), c.POINTER(c.c_int)
        L.lns_rollout_latent_ensemble_eval.argtypes = [vp, vp, vp, vp, i, i, i, ip, i, sp, vp, vp, vp, vp, vp, vp, vp, c.c_size_t, vp]
        L.lns_op_ensemble_score.argtypes = [vp, vp, i, i, i, i, i, i, sp, vp, vp, vp, vp, vp]
    if hasattr(L, "lns_rollout_latent_ensemble_quantiles"):
        sp, ip, qp = c.POINTER(LnsEvalSpec), c.POINTER(c.c_int), c.POINTER(LnsEnsembleQuantileSpec)
        L.lns_rollout_latent_ensemble_quantiles.argtypes = [vp, vp, vp, i, i, i, ip, i, qp, sp, vp, vp, vp, vp, vp, vp, c.c_size_t, vp]
        L.lns_op_ensemble_quantiles.argtypes = [vp, i, i, i, i, i, i, qp, sp, vp, vp, vp]
    if hasattr(L, "lns_rollout_latent_ensemble_exceed"):
        sp, ip, xp = c.POINTER(LnsEvalSpec), c.POINTER(c.c_int), c.POINTER(LnsEnsembleExceedSpec)
        L.lns_rollout_latent_ensemble_exceed.argtypes = [vp, vp, vp, vp, i, i, i, ip, i, xp, sp, vp, vp, vp, vp, vp, c.c_size_t, vp]
        L.lns_op_ensemble_exceed.argtypes = [vp, vp, i, i, i, i, i, i, xp, sp, vp, vp]
    if hasattr(L, "lns_rollout_latent_ensemble_analysis"):
        sp, ip, i64, dbl = c.POINTER(LnsEvalSpec), c.POINTER(c.c_int), c.c_int64, c.c_double
        L.lns_rollout_ensemble_analysis_workspace_bytes.argtypes = [vp, i, i, i, c.POINTER(c.c_size_t)]
        L.lns_rollout_latent_ensemble_analysis.argtypes = [vp, vp, vp, vp, vp, i64, i64, i, i, i, ip, i, sp, dbl, vp,
                                                           vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, c.c_size_t, vp]
        L.lns_op_ensemble_obs_gram.argtypes = [vp, vp, vp, i64, i64, i, i, i, i, i, i, sp, vp, vp, vp, vp]
        L.lns_op_etkf_transform.argtypes = [vp, vp, i, i, i, dbl, vp, vp, vp, vp, vp]
        L.lns_op_ensemble_transform.argtypes = [vp, vp, i, i, i64, vp, vp]
    if hasattr(L, "lns_rollout_latent_ensemble_analysis_local"):
        sp, ip, i64, dbl = c.POINTER(LnsEvalSpec), c.POINTER(c.c_int), c.c_int64, c.c_double
        L.lns_rollout_ensemble_analysis_local_workspace_bytes.argtypes = [vp, i, i, i, c.POINTER(c.c_size_t)]
        L.lns_rollout_latent_ensemble_analysis_local.argtypes = [vp, vp, vp, vp, vp, i64, i64, i, i, i, ip, i, sp, dbl, dbl, i, i, vp,
                                                                 vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                                                 vp, c.c_size_t, vp]
        L.lns_op_ensemble_patch_gram.argtypes = [vp, vp, vp, i64, i64, i, i, i, i, i, i, i, i, sp, vp, vp]
        L.lns_op_letkf_combine.argtypes = [vp, i, i, i, i, i, dbl, i, i, vp, vp, vp, vp, vp, vp]
        L.lns_op_ensemble_transform_local.argtypes = [vp, vp, i, i, i, i, i, vp, vp]
    if hasattr(L, "lns_rollout_eval_spectrum"):
        sp, ip = c.POINTER(LnsEvalSpec), c.POINTER(c.c_int)
        L.lns_spectrum_bins.argtypes = [i, i]
        L.lns_rollout_eval_spectrum.argtypes = [vp, vp, vp, vp, i, i, sp, vp, vp, ip, i, vp, vp, c.c_size_t, vp, ip, i, vp]
        L.lns_rollout_latent_eval_spectrum.argtypes = [vp, vp, vp, vp, i, i, i, i, sp, vp, vp, ip, i, vp, vp, vp, c.c_size_t, vp,
                                                       ip, i, vp]
        L.lns_op_energy_spectrum.argtypes = [vp, vp, i, i, i, i, i, sp, vp, vp]
    if hasattr(L, "lns_op_energy_spectrum_basis"):
        L.lns_spectrum_bins_basis.argtypes = [i, i, i, i]
        L.lns_op_energy_spectrum_basis.argtypes = [vp, vp, i, i, i, i, i, c.POINTER(LnsEvalSpec), vp, vp, i, i]
    if hasattr(L, "lns_rollout_eval_stats"):
        sp, ip, hp = c.POINTER(LnsEvalSpec), c.POINTER(c.c_int), c.POINTER(LnsStatsSpec)
        L.lns_rollout_eval_stats.argtypes = [vp, vp, vp, vp, i, i, sp, vp, vp, ip, i, vp, vp, c.c_size_t, vp, ip, i, vp,
                                             ip, i, hp, vp, vp]
        L.lns_rollout_latent_eval_stats.argtypes = [vp, vp, vp, vp, i, i, i, i, sp, vp, vp, ip, i, vp, vp, vp, c.c_size_t, vp,
                                                    ip, i, vp, ip, i, hp, vp, vp]
        L.lns_op_field_stats.argtypes = [vp, vp, i, i, i, i, i, sp, hp, vp, vp, vp]
    if hasattr(L, "lns_rollout_eval_maps"):
        sp, ip, qp = c.POINTER(LnsEvalSpec), c.POINTER(c.c_int), c.POINTER(LnsEvalSelect)
        L.lns_rollout_eval_maps_workspace_bytes.argtypes = [vp, i, c.POINTER(c.c_size_t)]
        L.lns_rollout_eval_maps.argtypes = [vp, vp, vp, vp, i, i, sp, vp, vp, ip, i, vp, vp, c.c_size_t, vp, qp]
        L.lns_rollout_latent_eval_maps.argtypes = [vp, vp, vp, vp, i, i, i, i, sp, vp, vp, ip, i, vp, vp, vp, c.c_size_t, vp, qp]
        L.lns_time_maps_state_bytes.argtypes = [i, i, i, i, c.POINTER(c.c_size_t)]
        L.lns_op_time_maps.argtypes = [vp, vp, i, i, i, i, i, sp, i, i, vp, vp, c.c_size_t, vp]
    if hasattr(L, "lns_rollout_eval_attrib"):
        sp, ip, ap = c.POINTER(LnsEvalSpec), c.POINTER(c.c_int), c.POINTER(LnsEvalAttrib)
        L.lns_rollout_eval_attrib_workspace_bytes.argtypes = [vp, i, c.POINTER(c.c_size_t)]
        L.lns_rollout_eval_attrib.argtypes = [vp, vp, vp, vp, i, i, sp, vp, vp, ip, i, vp, ap, vp, c.c_size_t, vp]
        L.lns_rollout_latent_eval_attrib.argtypes = [vp, vp, vp, vp, i, i, i, i, sp, vp, vp, ip, i, vp, vp, ap, vp, c.c_size_t, vp]
        L.lns_autoencode_eval_workspace_bytes.argtypes = [vp, i, c.POINTER(c.c_size_t)]
        L.lns_autoencode_eval.argtypes = [vp, vp, vp, i, i, sp, vp, vp, vp, vp, c.c_size_t, vp]
        L.lns_op_eval_attrib.argtypes = [vp, vp, vp, i, i, i, i, i, sp, vp, vp, vp, vp, vp]
        L.lns_op_latent_err.argtypes = [vp, vp, i, i, i, c.c_int64, c.c_float, vp, vp, vp]
    if hasattr(L, "lns_rollout_eval_flow"):
        sp, ip, qp = c.POINTER(LnsEvalSpec), c.POINTER(c.c_int), c.POINTER(LnsEvalSelect)
        fp_, wp = c.POINTER(LnsFlowSpec), c.POINTER(LnsEvalFlow)
        L.lns_rollout_eval_flow.argtypes = [vp, vp, vp, vp, i, i, sp, vp, vp, ip, i, vp, vp, c.c_size_t, vp, qp, wp]
        L.lns_rollout_latent_eval_flow.argtypes = [vp, vp, vp, vp, i, i, i, i, sp, vp, vp, ip, i, vp, vp, vp, c.c_size_t, vp, qp, wp]
        L.lns_op_flow_stats.argtypes = [vp, vp, i, i, i, i, i, sp, fp_, vp, vp, vp]
        L.lns_op_vorticity.argtypes = [vp, i, i, i, i, i, sp, fp_, vp, vp]
    if hasattr(L, "lns_check_finite"):      # (absent from older builds loaded through LNS_HIP_LIB for A/B runs)
        L.lns_check_finite.argtypes = [vp, i, vp, c.c_size_t, vp]
    if hasattr(L, "lns_set_option"):
        L.lns_set_option.argtypes = [vp, c.c_char_p, c.c_long]
    if hasattr(L, "lns_train_forward"):
        L.lns_train_workspace_bytes.argtypes = [vp, i, i, i, i, c.POINTER(c.c_size_t)]
        L.lns_train_forward.argtypes = [vp, vp, vp, vp, i, i, i, i, vp, vp, c.c_size_t, vp]
        L.lns_train_backward.argtypes = [vp, vp, vp, vp, vp, i, i, i, i, vp, vp, vp, c.c_size_t, vp]
    if hasattr(L, "lns_train_step"):
        ap = c.POINTER(LnsAdamSpec)
        L.lns_loss_smooth_l1.argtypes = [vp, vp, c.c_int64, c.c_float, vp, vp, vp, c.c_size_t, vp]
        L.lns_adam_step.argtypes = [vp, vp, vp, vp, vp, ap, vp]
        L.lns_adam_step_tensors.argtypes = [i, vp, vp, vp, vp, i64p, ap, vp]
        L.lns_train_step_workspace_bytes.argtypes = [vp, i, i, i, i, c.POINTER(c.c_size_t)]
        L.lns_train_step.argtypes = [vp, vp, vp, vp, vp, i, i, i, i, c.c_float, vp, vp, vp, ap, vp, vp, c.c_size_t, vp]
    if hasattr(L, "lns_train_step_clip"):
        up = c.POINTER(LnsUpdateSpec)
        L.lns_grad_norm_scratch_bytes.argtypes = [i, i64p, c.POINTER(c.c_size_t)]
        L.lns_grad_norm_tensors.argtypes = [i, vp, i64p, c.c_double, vp, vp, vp, c.c_uint32, vp, c.c_size_t, vp]
        L.lns_grad_scale_tensors.argtypes = [i, vp, i64p, vp, vp]
        L.lns_update_step_tensors.argtypes = [i, vp, vp, vp, vp, i64p, up, vp, vp]
        L.lns_train_step_clip_workspace_bytes.argtypes = [vp, i, i, i, i, c.POINTER(c.c_size_t)]
        L.lns_train_step_clip.argtypes = [vp, vp, vp, vp, vp, i, i, i, i, c.c_float, vp, vp, vp, up, vp, vp, vp, c.c_size_t, vp]
    if hasattr(L, "lns_fit_step"):
        ip, dp = c.POINTER(c.c_int), c.POINTER(c.c_double)
        L.lns_train_backward_ex.argtypes = [vp, vp, vp, vp, vp, i, i, i, i, vp, vp, vp, c.c_size_t, vp, vp]
        L.lns_loss_obs_mse_scratch_bytes.argtypes = [i, i, c.POINTER(c.c_size_t)]
        L.lns_loss_obs_mse.argtypes = [vp, vp, i, i, c.c_int64, i, ip, dp, vp, vp, c.c_double, vp, vp, vp, vp, vp, c.c_size_t, vp]
        L.lns_fit_step_workspace_bytes.argtypes = [vp, i, i, i, i, i, c.POINTER(c.c_size_t)]
        L.lns_fit_step.argtypes = [vp, vp, vp, vp, vp, vp, i, i, i, c.POINTER(LnsFitSpec), vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                   c.c_size_t, vp]
    if hasattr(L, "lns_train_tangent"):
        L.lns_train_tangent_workspace_bytes.argtypes = [vp, i, i, i, i, i, c.POINTER(c.c_size_t)]
        L.lns_train_tangent.argtypes = [vp, vp, i, i, i, i, i, i, i, vp, vp, vp, c.c_size_t, vp]
        L.lns_op_orthonormalize.argtypes = [vp, i, i, c.c_int64, vp, vp, vp]
    if hasattr(L, "lns_fit_gn_step"):
        ip, dp = c.POINTER(c.c_int), c.POINTER(c.c_double)
        L.lns_train_gn_product_workspace_bytes.argtypes = [vp, i, i, i, i, i, c.POINTER(c.c_size_t)]
        L.lns_train_gn_product.argtypes = [vp, vp, vp, vp, i, i, i, i, i, ip, dp, c.c_double, c.c_double, vp, vp, vp, vp, c.c_size_t, vp]
        L.lns_op_cg_start.argtypes = [vp, vp, vp, vp, i, c.c_int64, vp, vp, vp]
        L.lns_op_cg_update.argtypes = [vp, vp, vp, vp, vp, i, c.c_int64, c.c_double, vp, vp, vp, vp]
        L.lns_fit_gn_step_workspace_bytes.argtypes = [vp, i, i, i, i, i, c.POINTER(c.c_size_t)]
        L.lns_fit_gn_step.argtypes = [vp, vp, vp, vp, vp, vp, i, i, i, c.POINTER(LnsGnSpec), vp, vp, vp, vp, vp, c.c_size_t, vp]
    L.lns_build_has.argtypes = [c.c_char_p]
    L.lns_trace_enable.argtypes = [vp, i]
    L.lns_trace_count.argtypes = [vp]
    L.lns_trace_info.argtypes = [vp, i, c.c_char_p, i, i64p]
    L.lns_trace_copy.argtypes = [vp, i, vp]
    L.lns_timing_enable.argtypes = [vp, i]
    L.lns_timing_count.argtypes = [vp]
    L.lns_timing_info.argtypes = [vp, i, c.c_char_p, i, c.POINTER(c.c_double), i64p,
                                  c.POINTER(c.c_double), c.POINTER(c.c_double)]
    L.lns_timing_mfma_flops.argtypes = [vp, i, c.POINTER(c.c_double)]
    L.lns_op_conv2d.argtypes = [vp, i, i, i, i, i, i, vp, vp, i, i, i, i, i, i, i, i, i, i,
                                vp, i, i, vp, vp, vp, i, vp, vp]
    if hasattr(L, "lns_op_conv_gn"):
        L.lns_op_conv_gn.argtypes = [c.POINTER(LnsConvGnArgs), vp]
    if hasattr(L, "lns_op_fa_fused"):
        L.lns_op_fa_fused.argtypes = [c.POINTER(LnsFaFusedArgs), vp]
    if hasattr(L, "lns_op_fa_reducer"):
        L.lns_op_fa_reducer.argtypes = [c.POINTER(LnsFaReducerArgs), vp]
        L.lns_fa_reducer_fits.argtypes = [i, i, i, i]
        L.lns_op_fa_lrk.argtypes = [c.POINTER(LnsFaLrkArgs), vp]
        L.lns_fa_lrk_fits.argtypes = [i, i]
        L.lns_rotary_table.argtypes = [i, vp, i, vp]
        L.lns_op_ln_pe.argtypes = [vp, c.c_int64, i, i, i, vp, vp, vp, i, c.c_float, vp, fp, vp]
        L.lns_op_apply.argtypes = [vp, c.c_int64, vp, i, i, i, i, vp, vp, vp]
    if hasattr(L, "lns_op_conv_wgrad"):
        L.lns_op_conv_wgrad_scratch_bytes.argtypes = [i, i, i, i, i, i, i, c.POINTER(c.c_size_t)]
        L.lns_op_conv_wgrad.argtypes = [vp, vp, i, i, i, i, i, i, i, i, i, i, i, vp, vp, c.c_size_t, vp]
    if hasattr(L, "lns_op_groupnorm_train"):
        L.lns_op_groupnorm_train.argtypes = [vp, i, i, i, i, c.c_float, vp, vp, vp, vp, vp, vp, vp, vp, vp, i, vp, vp]
        L.lns_op_gelu_grad.argtypes = [vp, vp, vp, c.c_int64, vp]
        L.lns_op_bias_grad.argtypes = [vp, i, i, i, vp, i, vp]
    L.lns_op_groupnorm_stats.argtypes = [vp, i, i, i, i, c.c_float, vp, vp, vp, vp, vp]
    L.lns_op_attention.argtypes = [vp, i, i, i, i, c.c_float, vp, vp]
    L.lns_op_fa_sandwich.argtypes = [vp, vp, vp, i, i, i, i, i, c.c_float, i, vp, vp]
    L.lns_op_fa_pool.argtypes = [vp, c.c_int64, vp, i, i, i, i, vp, vp, vp]
    L.lns_op_fourier_block.argtypes = [vp, i, i, i, i, i, i, i, vp, vp, vp, vp, vp, vp, vp, vp, vp, i, i, vp, vp]
    L.lns_fourier_block_create.argtypes = [i, i, i, i, vp, vp, vp, vp, vp, vp, vp, vp, i, i, i, c.POINTER(vp)]
    L.lns_fourier_block_forward.argtypes = [vp, vp, vp, i, i, i, vp, vp]
    L.lns_fourier_block_destroy.argtypes = [vp]
    L.lns_fourier_block_destroy.restype = None
    L.lns_metric_rel_l2.argtypes = [vp, vp, i, i, i, i, c.c_float, c.c_float, c.c_float, vp, vp, vp, vp]
    L.lns_metric_rel_l2.restype = i
    L.lns_metric_rel_l2_ch.argtypes = [vp, vp, i, i, i, i, i, vp, vp, vp, c.c_float, c.c_float, c.c_float, vp, vp, vp, vp]
    L.lns_metric_rel_l2_ch.restype = i
    _lib = L
    return L

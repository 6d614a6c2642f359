/*
 * lns.h -- C ABI of the MI355X-native LNS rollout engine (liblns_hip.so).
 *
 * Drop-in boundary for ONE hot path of BaratiLab/LNS-Latent-Neural-PDE-Solver:
 *     LatentDynamics.predict(x, steps[, param], to_x)      train_stage2_ns2d.py:143-158
 *         = SimpleAutoencoder.encode                          modules/autoencoder2d.py:174-177
 *         -> steps x ( SimpleCNN.forward                      train_stage2_ns2d.py:82-87
 *                      ; SimpleAutoencoder.decode )           modules/autoencoder2d.py:179-182
 * (and the SW / two-phase / conditional variants of the same three functions).
 *
 * The reference has NO FFI/plugin layer of its own (it is 100% Python/PyTorch,
 * SURVEY.md F1), so there is no foreign interface to mirror symbol-for-symbol:
 * each entry point below names the reference Python method it replaces.  The
 * ABI is plain C: opaque handle, plain pointers and sizes, int status codes,
 * no C++/torch types.  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - all tensors are fp32, NCHW, contiguous unless a batch stride is given;
 *   - `x`, `z`, `y`, `out`, `param`, `workspace` are DEVICE pointers owned by
 *     the caller (e.g. torch `data_ptr()`); weights passed to lns_set_weight
 *     are HOST pointers;
 *   - `stream` is a hipStream_t (void*), e.g. torch.cuda.current_stream().cuda_stream;
 *     calls are asynchronous with respect to the host;
 *   - every function returns 0 on success, a negative LNS_E* code otherwise and
 *     never throws; lns_last_error() gives the message;
 *   - an engine handle is not thread-safe; use one handle per GPU.
 *   - device memory is allocated only by lns_finalize_weights() (packed weights)
 *     and lns_prepare() (per-shape launch plans: index maps / rotary tables);
 *     the run calls use caller-provided workspace only.
 */
#ifndef LNS_H_
#define LNS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LNS_ABI_VERSION 2
#define LNS_MAX_STAGES 8
#define LNS_MAX_KEY 160

/* status codes */
#define LNS_OK 0
#define LNS_EINVAL (-1)     /* bad argument / unsupported configuration */
#define LNS_ENOKEY (-2)     /* unknown state_dict key / shape mismatch   */
#define LNS_ESTATE (-3)     /* call order (weights not finalized, ...)   */
#define LNS_ENOMEM (-4)     /* workspace too small / device alloc failed */
#define LNS_EHIP (-5)       /* HIP runtime error                         */
#define LNS_ENONFINITE (-6) /* lns_check_finite: a tensor of the last run holds inf / NaN */

/* autoencoder flavour: which reference file the AE follows */
#define LNS_AE_NONE 0
#define LNS_AE_SQUARE 1         /* modules/autoencoder2d.py                 */
#define LNS_AE_NONSQUARED 2     /* modules/autoencoder2d_nonsquared.py      */
#define LNS_AE_HALF_PERIODIC 3  /* modules/autoencoder2d_half_periodic.py   */

/* propagator flavour */
#define LNS_PROP_NONE 0
#define LNS_PROP_PLAIN 1        /* SimpleCNN, train_stage2_{ns2d,SW,twophase}.py:56-87        */
#define LNS_PROP_CONDITIONAL 2  /* SimpleCNN, train_stage2_twophase_conditional.py:78-121      */

/* per-axis boundary handling of the 'same' convolutions */
#define LNS_PAD_ZEROS 0
#define LNS_PAD_CIRCULAR 1

/* Flat mirror of the YAML keys the reference reads from `args`
 * (modules/autoencoder2d.py:19-27,78-92; train_stage2_ns2d.py:94-104). */
typedef struct lns_config {
    int32_t abi_version;            /* = LNS_ABI_VERSION */
    int32_t ae_kind;                /* LNS_AE_*   */
    int32_t prop_kind;              /* LNS_PROP_* */
    int32_t in_channels;
    int32_t latent_dim;
    int32_t Ly, Lx;                 /* output field size            */
    int32_t res_h, res_w;           /* `resolution` / `resolutions` */
    int32_t latent_resolution;
    int32_t ae_pad_y, ae_pad_x;     /* LNS_PAD_* of AE convs (is_periodic / periodic_direction) */
    int32_t n_encoder_channels;
    int32_t encoder_channels[LNS_MAX_STAGES];
    int32_t encoder_res_blocks;
    int32_t use_attn_enc;
    int32_t n_decoder_channels;
    int32_t decoder_channels[LNS_MAX_STAGES];
    int32_t decoder_res_blocks;
    int32_t n_attn_resolutions;
    int32_t attn_resolutions[LNS_MAX_STAGES];
    int32_t n_fourier_resolutions;
    int32_t fourier_resolutions[LNS_MAX_STAGES];
    int32_t use_fa;
    int32_t final_smoothing;
    int32_t disable_coarse_attn;
    int32_t attn_heads;
    int32_t attn_dim;
    float hw_ratio;                 /* nonsquared / half-periodic AEs */
    int32_t prop_n_block;
    int32_t prop_n_embd;
    int32_t prop_dilation;
    int32_t prop_pad_y, prop_pad_x; /* LNS_PAD_* of the propagator's 3x3 convs */
    int32_t cond_emb_dim;           /* conditional propagator only */
    char ae_prefix[32];             /* state_dict prefix of the AE: "vq_ae." / "ae." / "" */
    char prop_prefix[32];           /* "propagator." / ""                                 */
    /* ABI 2: ConditionalSimpleAutoencoder (modules/autoencoder2d_nonsquared.py:279-305): the encoder is CondEncoder
     * (:71-145, CondResidualBlock modules/cond_utils.py:58-128) and encode takes `param`; LNS_AE_NONSQUARED only */
    int32_t cond_encoder;
    int32_t cond_emb_channels;
} lns_config;

typedef struct lns_engine lns_engine;

/* message of the last failed lns_create() on this thread */
const char* lns_create_error(void);

/* Build the layer program for `cfg` (replaces LatentDynamics.__init__ /
 * SimpleAutoencoder.__init__ / SimpleCNN.__init__: train_stage2_ns2d.py:91-104,
 * modules/autoencoder2d.py:161-167, train_stage2_ns2d.py:57-80).  No GPU needed. */
int lns_create(const lns_config* cfg, lns_engine** out);
void lns_destroy(lns_engine* e);
const char* lns_last_error(const lns_engine* e);

/* Parameter table = the reference's state_dict() keys and shapes. */
int lns_num_params(const lns_engine* e);
int lns_param_info(const lns_engine* e, int index, char* key, int key_capacity,
                   int64_t* shape /* [8] */, int* ndim, int* is_buffer);

/* load_state_dict(): copy one tensor (HOST pointer, fp32, contiguous). */
int lns_set_weight(lns_engine* e, const char* key, const float* host_data,
                   const int64_t* shape, int ndim);
/* Repack all weights into kernel-native layout and upload to HIP device `device`. */
int lns_finalize_weights(lns_engine* e, int device);

/* Scheduling options of the rollout (they change HOW the launch sets are issued, never a bit of the result):
 *   "decode_group"    steps decoded by one launch set at batch B * k (default 1; 0 = automatic: about 256 samples per
 *                     launch set.  Measured on NS2d-128 B=64: k = 4 cuts the serial kernel time 11 % and the launches
 *                     2x but the overlapped rollout is 2 % slower than k = 1, tools/sched_sweep.py)
 *   "decode_streams"  decode streams of the overlapped rollout (1..4)
 *   "overlap"         1: latent chain on a side stream, decodes round-robin on the decode streams; 0: one stream
 *   "prop_priority"   1: the side stream of the latent chain is created with the highest stream priority
 *   "fa_chunk_mb"     FABlock2D: in_proj -> sandwich -> to_out are issued per group of samples whose 512-plane tensor is at
 *                     most this many MB (it then stays in the 256 MB Infinity Cache between the three kernels instead of going
 *                     to HBM three times); 0 = whole batch per launch.  Cached plans are rebuilt.  Default: LNS_FA_CHUNK_MB
 *   "fa_fused_gpb"    plane groups (of 16) one block of the fused FABlock kernel walks; 0 = automatic.  Cached plans are rebuilt.
 *   "eval_max_steps"  longest horizon of lns_rollout_eval / lns_rollout_latent_eval (it sizes their partial sums; default 1024)
 *   "track_nonfinite" 1: lns_check_finite also remembers the plan runs whose amax record has been reused since (the
 *                     earlier steps / decode groups of a rollout): one extra one-block launch per plan run (default 0)
 *   "train_wgrad"     weight-gradient kernel of lns_train_backward (and through it of lns_train_step and the drop-in's autograd
 *                     path).  0 (default): one block per 64 x 64 output tile (and tap) walks the whole K = batch x pixels;
 *                     1: batch-parallel -- K is cut into S slices of whole (sample, 64-pixel chunk)s, one block per (tile, slice),
 *                     3x3: all nine taps per block; the S partial tiles are summed in ascending slice order by a second kernel
 *                     (no atomics: bit-reproducible for a shape; the gradient differs from form 0 by the summation order only).
 *                     With 1 the training workspaces grow by one partial-sum area (see lns_train_workspace_bytes); any other
 *                     value: LNS_EINVAL.
 * Two options select an ARITHMETIC FORM (results differ at rounding level, ~2e-7 relative on the decoded field):
 *   "fa_fused"        2 (default; LNS_FA_FUSED): FABlock2D on 64 x 64 planes with 64 channels and on 32 x 32 planes with 128
 *                     channels computes in_proj inside the sandwich kernel (csrc/fa_fused.inc) -- the heads * dim_head plane tensor
 *                     is never stored; 1 / 3: other forms of the 64 x 64 kernel (single-buffered band image / the generic kernel:
 *                     same bits as 2, slower); 0: in_proj as its own 1x1 convolution, then the sandwich.  Cached plans are rebuilt.
 *   "fold_linear"     1 (default; LNS_NO_FOLD_LINEAR=1 in the environment makes it 0): a convolution directly followed by a 1x1
 *                     convolution -- no norm, activation or residual between them -- runs as ONE convolution on weights composed
 *                     when the weights are finalized (W' = W2 W1, b' = W2 b1 + b2; csrc/lns_fold.h): the decoder's output layer
 *                     3x3 -> 1x1 and post_quant_conv -> decoder.model.0 of the square autoencoder, the encoder's last
 *                     1x1 -> quant_conv.  The parameter table is unchanged; the layer trace shows the pair under the 1x1's name.
 *                     0: the pair as two launches, or as the 64 -> 64 1x1 in the first convolution's epilogue.  Any other
 *                     value: LNS_EINVAL.  Cached plans are rebuilt.
 *   "up2_dual"        1 (default; LNS_UP2_DUAL=0 in the environment makes it 0): a 3x3 convolution behind an exactly-2x nearest
 *                     upsample takes the dual-phase form (csrc/conv3_up2d.inc: one block per source tile and row phase computes
 *                     both column phases and stores pixel pairs) wherever that form fits -- a per-layer rule; 0: the per-phase
 *                     form everywhere, launch for launch the plan without the form.  The results have the same bits either way.
 *                     Any other value: LNS_EINVAL.  Cached plans are rebuilt.
 * One option selects WHICH RESULT is computed (a third kind: no scheduling option interacts with it, and it changes no
 * workspace size):
 *   "spectrum_basis"  basis of the energy spectra of the streaming calls (the _spectrum, _stats and _maps entry points and
 *                     their _latent_ forms): basis_y | basis_x << 1 with LNS_SPECTRUM_DFT (0) or LNS_SPECTRUM_DCT (1) per
 *                     axis; default 0 (DFT on both axes, the bits of the library without the option).  It is read when a
 *                     call is enqueued; spectra_out then holds S = lns_spectrum_bins_basis(Ly, Lx, basis_y, basis_x) bins.
 *                     Outside 0 .. 3: LNS_EINVAL (host only, nothing is touched).
 * Defaults come from LNS_DECODE_GROUP / LNS_DECODE_STREAMS / LNS_NO_OVERLAP / LNS_PROP_PRIORITY at lns_create().
 * Changing an option changes the workspace size: call lns_prepare() again. */
int lns_set_option(lns_engine* e, const char* name, long value);

/* Latent shape for the configured field size: z is [B, C, H, W]. */
int lns_latent_shape(const lns_engine* e, int* C, int* H, int* W);

/* Build (and cache) launch plans for batch B; returns the workspace bytes the run
 * calls need for that batch through *workspace_bytes (may be NULL). */
int lns_prepare(lns_engine* e, int B, size_t* workspace_bytes);

/* SimpleAutoencoder.encode: x [B,Cin,Ly,Lx] -> z [B,latent_dim,h,w]. */
int lns_encode(lns_engine* e, const float* x, int B, float* z,
               void* workspace, size_t workspace_bytes, void* stream);
/* ConditionalSimpleAutoencoder.encode(x, param) (cfg.cond_encoder = 1): param [B] device, one value per sample. */
int lns_encode_cond(lns_engine* e, const float* x, const float* param, int B, float* z,
                    void* workspace, size_t workspace_bytes, void* stream);
/* encode(x * scale + shift) with the affine map applied in the first convolution's prologue (device table
 * scale_shift [B][in_channels][2]): the dataset normalisation (u - mean) / (std + eps) of the reference's encode_dataset
 * (dataset/ns2d_fno_stage2_simpleae.py:78-93, dataset/Stage2_SW.py:74-105, dataset/twophase_flow_stage2.py:304-337)
 * without a normalised copy of the frames.  param: NULL, or [B] for a conditional encoder. */
int lns_encode_affine(lns_engine* e, const float* x, const float* scale_shift, const float* param, int B, float* z,
                      void* workspace, size_t workspace_bytes, void* stream);
/* SimpleAutoencoder.decode: z [B,latent_dim,h,w] -> y [B,Cin,Ly,Lx]. */
int lns_decode(lns_engine* e, const float* z, int B, float* y,
               void* workspace, size_t workspace_bytes, void* stream);
/* SimpleCNN.forward: z_in [B,latent_dim,H,W] (+ param [B] or NULL) -> z_out (same shape). */
int lns_propagate(lns_engine* e, const float* z_in, const float* param, int B, int H, int W,
                  float* z_out, void* workspace, size_t workspace_bytes, void* stream);
/* LatentDynamics.predict(x, T[, param], to_x): out is [B,T,Cin,Ly,Lx] if to_x else
 * [B,T,latent_dim,h,w]; latents_out (nullable) additionally receives [B,T,latent_dim,h,w]. */
int lns_rollout(lns_engine* e, const float* x, const float* param, int B, int T, int to_x,
                float* out, float* latents_out, void* workspace, size_t workspace_bytes,
                void* stream);

/* The same loop started from a latent state (chunked rollouts, e.g. to overlap the
 * gather of finished step blocks with the remaining steps): z_in [B,latent_dim,h,w] ->
 * out [B,T,...]; z_last (nullable) receives the latent after step T. */
int lns_rollout_latent(lns_engine* e, const float* z_in, const float* param, int B, int T, int to_x,
                       float* out, float* z_last, void* workspace, size_t workspace_bytes, void* stream);

/* ---- selected-step rollout: decode only the steps the caller keeps ---------------------------------------------
 * lns_rollout(..., to_x = 1) for a caller that looks at a few of the T steps (the reference's validation loop plots
 * y_hat[:10, ::5, 0], train_stage2_ns2d.py:259-263): the latent chain runs all T steps, the decoder runs for the kept
 * steps only.  keep_steps_host: n_keep >= 1 strictly ascending 0-based steps in [0, T) (HOST array, read during the
 * call).  out is [B,n_keep,Cin,Ly,Lx] and out[:, i] holds the bits lns_rollout writes to out[:, keep_steps[i]], whatever
 * the scheduling options: a decode group is the next up to "decode_group" KEPT steps, decoded by the launch set of the
 * full rollout at batch B * (steps in the group).  latents_out (nullable) is the full [B,T,latent_dim,h,w]: every latent
 * is computed anyway.  Decoded fields only (no to_x): for latents, slice lns_rollout(..., to_x = 0).
 * param, batch limits, trace / timing modes (single stream) and lns_check_finite: as for lns_rollout.
 * LNS_EINVAL (bad argument, named by lns_last_error; decided before any device work), LNS_ENOMEM (workspace smaller
 * than lns_rollout_select_workspace_bytes; nothing is enqueued), LNS_ESTATE (no autoencoder / propagator).
 *
 * Workspace for batch B: the lns_prepare(B) layout, byte for byte (lns_prepare and the sizes the other run calls need
 * do not change), rounded up to 256 bytes, followed by two latent buffers of B * latent_dim * h * w floats, each rounded
 * up to 256 bytes: the chain writes the latent of a skipped step into them alternately (it cannot write a step into
 * the buffer it reads), the latent of a kept step into the ring of the rollout layout. */
int lns_rollout_select_workspace_bytes(lns_engine* e, int B, size_t* bytes);
int lns_rollout_select(lns_engine* e, const float* x, const float* param, int B, int T,
                       const int* keep_steps_host, int n_keep, float* out, float* latents_out,
                       void* workspace, size_t workspace_bytes, void* stream);
/* The same from a latent state (lns_rollout_latent; chunked rollouts): keep_steps_host are steps of THIS chunk,
 * 0 .. T-1; z_last (nullable) receives the latent after step T. */
int lns_rollout_latent_select(lns_engine* e, const float* z_in, const float* param, int B, int T,
                              const int* keep_steps_host, int n_keep, float* out, float* z_last,
                              void* workspace, size_t workspace_bytes, void* stream);

/* ---- ensemble rollout: per-step mean and variance over perturbed members ---------------------------------------
 * The reference trains the propagator with noise on the latent (z_in + randn_like(z_in) * noise_level,
 * train_stage2_ns2d.py:211-212) so that LatentDynamics.predict (train_stage2_ns2d.py:143-158) tolerates a perturbed
 * latent; the inference-side use is an ensemble forecast: encode once, perturb the latent M times (the caller's one
 * torch op, as for training), roll every member out and keep the mean and the spread per step -- without the
 * [B*M,T,Cin,Ly,Lx] tensor of lns_rollout_latent at batch B*M and without a second pass over it.
 * The chain runs at batch N = B*M (launch sample b*M + m is member m of trajectory b); the kept steps have the semantics
 * of lns_rollout_latent_select (a decode group is the next up to "decode_group" kept steps, resolved for N); the decode
 * of a group writes a per-decode-stream frame buffer [steps][B][M][Cin*Ly*Lx], and a reduction kernel on the same
 * stream writes mean_out[b][i] and var_out[b][i] before the buffer is reused.  Per element, in fp32, nothing fused:
 *     s = f[0]; for m = 1 .. M-1: s = s + f[m];   mean = s / (float)M
 *     d_m = f[m] - mean;  sd = sum_m d_m;  q = sum_m d_m * d_m            (ascending m)
 *     var = (q - sd * sd / (float)M) / (float)(M - 1)                     (unbiased; corrected two-pass form)
 * so a result depends on its M member values only, never on the scheduling options; f[m] are the bits lns_rollout_latent
 * at batch B*M writes for sample b*M + m.  M = 1: mean is the rollout itself, var_out must be NULL.
 * There is no from-x form and no device random numbers: encoding is one lns_encode call, the noise the caller's.
 * param, batch limits (on B*M), trace / timing modes (single stream) and lns_check_finite (with B*M): as for lns_rollout.
 * LNS_EINVAL (bad argument, named by lns_last_error; decided before any device work), LNS_ENOMEM (workspace smaller than
 * lns_rollout_ensemble_workspace_bytes; nothing is enqueued), LNS_ESTATE (no autoencoder / propagator).
 *
 * Workspace for (B, M), N = B*M: the lns_prepare(N) layout, byte for byte (lns_prepare and the sizes the other run calls
 * need do not change), followed by two regions, each rounded up to 256 bytes: the two latent buffers of
 * lns_rollout_select_workspace_bytes(N), then "decode_streams" frame buffers of decode_group * N * Cin * Ly * Lx * 4
 * bytes (decode_group as resolved for N when the option is 0). */
int lns_rollout_ensemble_workspace_bytes(lns_engine* e, int B, int M, size_t* bytes);
/* z_in [B][M][zper]; param [B][M] (one value per MEMBER: a parameter ensemble is the same call) or NULL;
 * mean_out, var_out (nullable) [B][n_keep][Cin][Ly][Lx]; z_last (nullable) [B][M][zper]; keep_steps_host as lns_rollout_latent_select */
int lns_rollout_latent_ensemble(lns_engine* e, const float* z_in, const float* param, int B, int M, int T,
                                const int* keep_steps_host, int n_keep, float* mean_out, float* var_out, float* z_last,
                                void* workspace, size_t workspace_bytes, void* stream);

/* ---- streaming validation rollout: predict and score without the [B,T] field ---------------------------------
 * Reference: the body of the validation loop, train_stage2_ns2d.py:249-263 (same text in train_stage2_SW.py and
 * train_stage2_twophase*.py, where denormalize is the per-channel / closed-wall / clamp form):
 *     y_hat = model.predict(x, T, to_x=True); y_hat, y = denormalize(y_hat), denormalize(y)
 *     frame_wise = relative_lp_loss(y_hat, y, reduce_dim=(3, 4)); seq_wise = relative_lp_loss(y_hat, y, reduce_dim=(1, 3, 4))
 * i.e. lns_rollout followed by lns_metric_rel_l2{,_ch}, without the decoded rollout [B,T,C,Ly,Lx] between them: the
 * decode of every group of steps writes a per-decode-stream frame buffer, a scoring kernel on the same stream reduces
 * it against the truth planes of those steps to the metric's per-plane sums, and the metric's finish kernel runs once
 * on the caller's stream after the streams have joined.  The per-plane arithmetic and reduction order are those of
 * lns_metric_rel_l2{,_ch} (one device function shared by the kernels), so frame_out / seq_out hold the bits the two
 * calls produce (for y_hat and y_true of equal 16-byte alignment, as any allocator gives), whatever the scheduling options.
 *
 * lns_eval_spec: the denormalisation, i.e. the arguments of lns_metric_rel_l2 (per_channel = 0: mean, std) or of
 * lns_metric_rel_l2_ch (per_channel = 1: mean_c / std_c / flags_c (LNS_METRIC_*) per channel, clamp_lo / clamp_hi;
 * in_channels <= 8), and eps for both.  size = sizeof(lns_eval_spec): another value is LNS_EINVAL. */
typedef struct lns_eval_spec {
    uint32_t size;
    int32_t per_channel;
    float mean, std, eps;
    float mean_c[8], std_c[8];
    int32_t flags_c[8];
    float clamp_lo, clamp_hi;
} lns_eval_spec;

/* Workspace of the two calls below for batch B: the lns_prepare(B) layout, byte for byte (lns_prepare and the sizes
 * the other run calls need do not change), followed by
 *     "decode_streams" frame buffers of decode_group * B * in_channels * Ly * Lx * 4 bytes   (decode_group as resolved
 *                                                                                             for B when the option is 0)
 *     the partial sums [B]["eval_max_steps"][in_channels][2] floats,
 * each rounded up to 256 bytes.  The horizon is bounded by the option "eval_max_steps" (lns_set_option; default 1024,
 * 1 .. 65536): T (T_total) above it is LNS_EINVAL.  NS2d 128 x 128 x 3, B = 64, three decode streams: 37.7 MB + 1.6 MB,
 * against the 805 MB (T = 64) / 3.22 GB (T = 256) of the rollout tensor.  Changing a scheduling option changes the size. */
int lns_rollout_eval_workspace_bytes(lns_engine* e, int B, size_t* bytes);

/* x [B,Cin,Ly,Lx], y_true [B,T,Cin,Ly,Lx] (normalised, like the decoded rollout) -> frame_out [B,T,Cin], seq_out [B,Cin]
 * (either may be NULL, not both).  keep_steps_host: n_keep ascending 0-based steps (HOST array, read during the call)
 * whose decoded frames are copied to frames_out [B,n_keep,Cin,Ly,Lx] -- the reference plots y_hat[:10, ::5, 0]
 * (train_stage2_ns2d.py:259-263); n_keep = 0: keep_steps_host / frames_out are ignored.
 * param, batch limits, trace / timing modes (single stream) and lns_check_finite: as for lns_rollout.
 * LNS_EINVAL (bad argument, named by lns_last_error; decided before any device work), LNS_ENOMEM (workspace smaller
 * than lns_rollout_eval_workspace_bytes), LNS_ESTATE (no autoencoder / propagator). */
int lns_rollout_eval(lns_engine* e, const float* x, const float* param, const float* y_true, int B, int T,
                     const lns_eval_spec* spec, float* frame_out, float* seq_out, const int* keep_steps_host, int n_keep,
                     float* frames_out, void* workspace, size_t workspace_bytes, void* stream);

/* The same from a latent state (lns_rollout_latent; chunked evaluations): scores steps t0 .. t0+T-1 of
 * y_true [B,T_total,Cin,Ly,Lx].  The per-plane sums of a chunk stay in `workspace` at their [B][T_total][Cin][2] slots;
 * the call that completes the horizon (t0 + T == T_total) runs the finish kernel and writes frame_out [B,T_total,Cin] and
 * seq_out [B,Cin]; earlier chunks leave them untouched.  The chunks of one evaluation must therefore use the same
 * workspace, and nothing else may write its evaluation part in between (lns_rollout & co. do not: they stay inside the
 * lns_prepare bytes).  keep_steps_host: steps of THIS chunk, 0 .. T-1.  z_last (nullable): the latent after step t0+T. */
int lns_rollout_latent_eval(lns_engine* e, const float* z_in, const float* param, const float* y_true, int B, int T,
                            int t0, int T_total, const lns_eval_spec* spec, float* frame_out, float* seq_out,
                            const int* keep_steps_host, int n_keep, float* frames_out, float* z_last, void* workspace,
                            size_t workspace_bytes, void* stream);

/* ---- ensemble validation: streaming CRPS, spread / skill and rank histograms -------------------------------------
 * lns_rollout_latent_ensemble with the members scored against the truth where they are decoded: is the spread calibrated
 * (spread against rmse), is the ensemble mean better than one forecast (rmse, rel_l2), does the truth fall inside the
 * members (rank histogram), and the fair CRPS -- all of which need the M member values and the truth of a pixel at the
 * same time, i.e. the [B*M, n_keep, Cin, Ly, Lx] tensor the ensemble call exists to avoid.  The chain, the kept steps, the
 * frame buffers and the workspace are those of lns_rollout_latent_ensemble; a scoring kernel follows the decode of a group
 * on its decode stream (one block per plane), and a finish kernel runs once on the caller's stream after the join.
 *
 * Every frame is denormalised as lns_eval_spec says, members and truth by the same map D_c of channel c:
 *     per_channel = 0:  D_c(x) = x * std + mean
 *     per_channel = 1:  x * std_c + mean_c, then 0 on the four wall rows / columns under flag 1, then
 *                       fminf(fmaxf(., clamp_lo), clamp_hi) under flag 2
 * For one pixel, v_m = D_c(f_m), q = D_c(y); fp32, nothing fused (the product and the sum of D_c included), m ascending:
 *     s = v_0; s = s + v_m (m = 1 .. M-1);  mu = s / (float)M
 *     d_m = v_m - mu;  sd = sum d_m;  qq = sum d_m * d_m;  var = (qq - sd * sd / (float)M) / (float)(M - 1)
 *     e = mu - q;  se = e * e;  g = q * q
 *     a = sum_m |v_m - q|
 *     w = 0; for m = 0 .. M-2: for n = m+1 .. M-1: w = w + |v_m - v_n|          (one running sum, in this order)
 *     crps = a / (float)M - w / (float)(M * (M - 1))                            (the fair CRPS)
 *     rank = #{ m : v_m < q }                                                   (0 .. M; a NaN compares false)
 * (sd, qq, a and w start from 0.)  Per plane (b, kept step i, c) four fp32 sums over its H * W pixels, SE = sum se, G = sum g,
 * V = sum var, CR = sum crps, in the order of the metric kernels: thread t of 256 adds pixels t, t + 256, ... in ascending
 * order, then the wave sum, then (w0 + w1) + (w2 + w3) over the four waves.  One block owns one plane, so every slot has one
 * writer: no float atomics, nothing depends on the grouping or the scheduling options.  The rank histogram of a plane is M + 1
 * int32 counts (integer LDS atomics: order-independent).  The finish kernel turns the sums, in place, into
 *     rel_l2 = sqrtf(SE / (G < eps ? eps : G)),  rmse = sqrtf(SE / HW),  spread = sqrtf(V / HW),  crps = CR / HW
 * (HW = (float)(H * W)) and, per (b, c), over the kept steps in ascending order, into seq_out:
 *     sqrtf(sum SE / (sum G < eps ? eps : sum G)),  sqrtf(sum SE / N),  sqrtf(sum V / N),  sum CR / N,   N = (float)(n_keep * H * W)
 * A calibrated ensemble has spread * sqrt((M + 1) / M) / rmse near 1.
 *
 * z_in, param, keep_steps_host, z_last, B, M, T: as lns_rollout_latent_ensemble, with 2 <= M <= 128.
 * y_true [B][n_keep][Cin][Ly][Lx]: the normalised truth of the KEPT steps.  mean_out / var_out (both nullable; var_out
 * needs mean_out): lns_rollout_latent_ensemble's outputs, same bits; the reduction kernel runs only when mean_out is given.
 * workspace: lns_rollout_ensemble_workspace_bytes(B, M), no more (the plane sums live in scores_out until the finish kernel).
 * Trace / timing modes, lns_check_finite (with B*M) and the status codes: as lns_rollout_latent_ensemble. */
int lns_rollout_latent_ensemble_eval(lns_engine* e, const float* z_in, const float* param, const float* y_true,
                                     int B, int M, int T, const int* keep_steps_host, int n_keep, const lns_eval_spec* spec,
                                     float* scores_out,   /* [B][n_keep][Cin][4]: rel_l2, rmse, spread, crps */
                                     float* seq_out,      /* nullable [B][Cin][4] */
                                     int32_t* rank_out,   /* nullable [B][n_keep][Cin][M+1] */
                                     float* mean_out, float* var_out, float* z_last,
                                     void* workspace, size_t workspace_bytes, void* stream);

/* ---- ensemble quantiles: per-pixel quantiles and exceedance probabilities over the members -----------------------
 * lns_rollout_latent_ensemble with, per kept step and pixel, quantiles of the M member values (a median, a 5-95 % band, the
 * envelope) and the probability that the field exceeds a threshold: what a forecast user without a truth takes from an
 * ensemble, and for a clamped or wall-zeroed channel what mean and variance do not say.  Each needs the M member values of
 * a pixel at the same time, i.e. the [B*M, n_keep, Cin, Ly, Lx] tensor the ensemble call exists to avoid.  The chain, the
 * kept steps, the frame buffers and the workspace are those of lns_rollout_latent_ensemble; a quantile kernel follows the
 * decode of a group on its decode stream (one pixel per thread, grid over pixel tiles and planes).
 *
 * The statement, for one pixel of plane (b, kept step i, channel c):
 *     v_m = D_c(f_m), D_c the map of lns_eval_spec as written above for lns_rollout_latent_ensemble_eval (product and sum
 *     rounded one by one, wall-zero and clamp flags included; eps unused); norm == NULL: v_m = f_m, in normalised units as
 *     mean_out is.
 *     The M values are sorted ascending by the total order of their IEEE bit patterns:
 *         key(x) = bits ^ (sign ? 0xFFFFFFFF : 0x80000000), compared as unsigned
 *     (-0 below +0, NaNs ordered by their sign): the sorted sequence v_(0) <= ... <= v_(M-1) is unique, any sorting algorithm
 *     gives the same bits.
 *     Quantile position of the probability p_k, 0 <= p <= 1, on the host in double:
 *         h = p (M - 1);  lo = floor(h);  frac = (float)(h - lo);  lo = M - 1 forces frac = 0
 *     Quantile value (numpy's and torch's "linear" definition), fp32, nothing fused:
 *         frac == 0:  Q_k = v_(lo)
 *         otherwise:  d = v_(lo+1) - v_(lo);  t = frac * d;  Q_k = v_(lo) + t
 *     so p = 0 is the member minimum and p = 1 the maximum.
 *     Exceedance probability of the threshold thr[k][c] (in the units of v):
 *         P_k = (float)#{m : v_m > thr[k][c]} / (float)M                        (a NaN compares false)
 * There is no reduction across pixels: no plane sums, no finish kernel, no atomics; a result depends on its M inputs only,
 * never on the grouping or the scheduling options.
 *
 * lns_ensemble_quantile_spec: n_q probabilities q[0 .. n_q) and n_thr thresholds thr[k][c], c < in_channels; size =
 * sizeof(lns_ensemble_quantile_spec) and reserved = 0. */
typedef struct lns_ensemble_quantile_spec {
    uint32_t size; int32_t n_q, n_thr; uint32_t reserved; /* 0 */
    double q[8];          /* probabilities in [0, 1] */
    float  thr[8][8];     /* thr[k][c], c < in_channels */
} lns_ensemble_quantile_spec;

/* z_in, param, keep_steps_host, z_last, B, M, T: as lns_rollout_latent_ensemble, with 1 <= M <= 128.
 * norm (nullable): the denormalisation; quant_out [B][n_keep][n_q][Cin][Ly][Lx] (needed when n_q > 0), prob_out
 * [B][n_keep][n_thr][Cin][Ly][Lx] (needed when n_thr > 0; in_channels <= 8); n_q, n_thr in 0 .. 8, not both 0.  mean_out / var_out (both
 * nullable; var_out needs mean_out and M >= 2): lns_rollout_latent_ensemble's outputs, same bits; the reduction kernel runs
 * only when mean_out is given.  workspace: lns_rollout_ensemble_workspace_bytes(B, M), no more.
 * Trace / timing modes, lns_check_finite (with B*M) and the status codes: as lns_rollout_latent_ensemble. */
int lns_rollout_latent_ensemble_quantiles(lns_engine* e, const float* z_in, const float* param, int B, int M, int T,
                                          const int* keep_steps_host, int n_keep, const lns_ensemble_quantile_spec* qspec,
                                          const lns_eval_spec* norm /* nullable */, float* quant_out, float* prob_out,
                                          float* mean_out, float* var_out, float* z_last,
                                          void* workspace, size_t workspace_bytes, void* stream);

/* ---- ensemble exceedance: contingency tables of the event "field above a threshold" --------------------------------
 * lns_rollout_latent_ensemble with the members' exceedance forecast P(field > threshold) verified against the truth where
 * the members are decoded.  The Brier score and its reliability / resolution / uncertainty split, the reliability diagram,
 * the ROC curve and its area, and for one forecast hits / misses / false alarms (the IoU of the region above the threshold)
 * are all functions of one integer table per plane: how many pixels had n of the M members above the threshold while the
 * truth was (o = 1) or was not (o = 0) above it.  Taking it needs the M member values and the truth of a pixel at the same
 * time, i.e. the [B*M, n_keep, Cin, Ly, Lx] tensor the ensemble call exists to avoid.  The chain, the kept steps, the frame
 * buffers and the workspace are those of lns_rollout_latent_ensemble; a counting kernel follows the decode of a group on its
 * decode stream (one pixel per thread, grid over pixel tiles and planes, as the quantile kernel).
 *
 * The statement, for one pixel of plane (b, kept step i, channel c) and threshold k:
 *     v_m = D_c(f_m), q = D_c(y), D_c the map of lns_eval_spec as written above for lns_rollout_latent_ensemble_eval (product
 *     and sum rounded one by one, wall-zero and clamp flags included; eps unused); norm == NULL: v_m = f_m and q = y, in
 *     normalised units.
 *         n = #{m : v_m > thr[k][c]}        (0 .. M)
 *         o = (q > thr[k][c]) ? 1 : 0
 *     thr[k][c] in the units of v; a NaN compares false in both comparisons.
 *     table[b][i][k][c][o][n] = the number of the plane's H * W pixels with that (o, n)
 * table_out is int32 [B][n_keep][n_thr][Cin][2][M+1]; every [b][i][k][c] slice sums to H * W (H * W <= 2^30 keeps a count
 * inside int32); there is nothing else in it and no floating point.  The call overwrites the whole table: the caller does
 * not zero it.  Counts are added with integer atomics (LDS per block, then one global add per non-zero bin); integer adds
 * commute and never round, so the table is the same bits whatever the grouping or the scheduling options, and there is no
 * finish kernel.  The scores are float64 functions of the table, taken on the host (the Python package: metrics.brier_scores,
 * reliability_curve, roc_curve, contingency_scores).
 *
 * lns_ensemble_exceed_spec: n_thr thresholds thr[k][c], c < in_channels; size = sizeof(lns_ensemble_exceed_spec). */
typedef struct lns_ensemble_exceed_spec {
    uint32_t size; int32_t n_thr;   /* 1 .. 8 */
    float thr[8][8];                /* thr[k][c], c < in_channels, in the units of v */
} lns_ensemble_exceed_spec;

/* z_in, param, keep_steps_host, z_last, B, M, T: as lns_rollout_latent_ensemble, with 1 <= M <= 128; in_channels <= 8.
 * y_true [B][n_keep][Cin][Ly][Lx]: the normalised truth of the KEPT steps, as for lns_rollout_latent_ensemble_eval.
 * norm (nullable): the denormalisation of members and truth.  mean_out / var_out (both nullable; var_out needs mean_out and
 * M >= 2): lns_rollout_latent_ensemble's outputs, same bits; the reduction kernel runs only when mean_out is given.
 * workspace: lns_rollout_ensemble_workspace_bytes(B, M), no more.
 * Trace / timing modes, lns_check_finite (with B*M) and the status codes: as lns_rollout_latent_ensemble. */
int lns_rollout_latent_ensemble_exceed(lns_engine* e, const float* z_in, const float* param, const float* y_true,
                                       int B, int M, int T, const int* keep_steps_host, int n_keep,
                                       const lns_ensemble_exceed_spec* xspec, const lns_eval_spec* norm /* nullable */,
                                       int32_t* table_out,   /* [B][n_keep][n_thr][Cin][2][M+1] */
                                       float* mean_out, float* var_out, float* z_last,
                                       void* workspace, size_t workspace_bytes, void* stream);

/* ---- ensemble transform Kalman filter on sparse, decoded observations --------------------------------------------
 * lns_rollout_latent_ensemble with the ensemble corrected by observations in PHYSICAL space: a few sensors, one observed
 * channel, a masked region.  An ensemble transform Kalman filter (ETKF; Hunt, Kostelich, Szunyogh 2007, without
 * localisation) needs no adjoint: it needs the decoded members at the observed steps -- the frame buffers of the ensemble
 * sink -- the M x M Gram matrix of their anomalies under the observation weights, a symmetric inverse square root of it, and
 * an M x M transform of the latent members.  The same transform updates a per-member param, so a parameter is estimated
 * from sparse decoded observations also where the encoder is conditional.
 *
 * Notation: M members, p runs over the Cin*Ly*Lx values of a frame, r_p >= 0 is the inverse observation-error variance of
 * value p (0: not observed).  rinv is fp32 and addressed as rinv + b * rinv_bs + i * rinv_ss + p for sample b and kept step i
 * (strides in floats, >= 0; 0: the map is shared).
 *
 * 1. Gram (per sample b and kept step i; double throughout):
 *     f_m = D_c(member m), y = D_c(y_obs): the map of lns_eval_spec as written for lns_rollout_latent_ensemble_eval (the one
 *     denormalisation device function of the scored kernels; norm == NULL: the values as they are), then converted to double
 *         ybar_p = (f_0 + f_1 + ... + f_{M-1}) / M          (m ascending)
 *         Y_m = f_m - ybar,   d = y - ybar,   w_m = r_p * Y_m
 *         S_ij = sum_p w_i Y_j   for i <= j,   S_ji = S_ij            g_i = sum_p w_i d
 *         stat = (sum_p (r_p d) d,  sum_p r_p,  #{p : r_p > 0})
 *     A value with !(r_p > 0) contributes nothing whatever y_obs and the members hold there (a select, not a product with 0:
 *     NaN and inf at unobserved values are harmless, and they are not read).
 *     Order: the frame is cut into slices of LNS_ETKF_SLICE = 1024 consecutive values p; inside a slice every sum starts at
 *     0 and takes one fused multiply-add per value, p ascending: acc = fma(w_i, Y_j, acc), fma(w_i, d, acc), fma(r_p d, d, acc)
 *     (sum r_p: plain adds; an unobserved value adds fma(0, 0, acc) or is skipped); then the slices are added in ascending
 *     order, starting from slice 0.  The slice length is a constant: the result depends on its inputs only, never on the
 *     grouping, the streams or any scheduling option.  No atomics.
 * 2. Transform (per sample; double, nothing fused):
 *     S_tot, g_tot: the sums over the n kept steps, ascending (the 4D form: the observations of several steps of one window
 *     give one set of weights).  A = dg I + S_tot with dg = (M - 1) / rho on the diagonal (dg + S_ii), rho >= 1 the
 *     multiplicative inflation.  Cyclic Jacobi, A = Q Lambda Q^T: a sweep is n' - 1 rounds over n' = M + (M & 1) indices in the
 *     round-robin order -- round r = 0 .. n' - 2 holds the n'/2 disjoint pairs {n' - 1, r} and, for k = 1 .. n'/2 - 1,
 *     {(r + k) mod (n' - 1), (r - k) mod (n' - 1)}; a pair with the padding index of an odd M rests.  For a pair p < q
 *     with a_pq != 0:  theta = (a_qq - a_pp) / (2 a_pq), t = sgn(theta) / (|theta| + sqrt(theta^2 + 1)), c = 1 / sqrt(t^2 + 1),
 *     s = t c, all from the matrix before the round; then rows (a_pj, a_qj) <- (c a_pj - s a_qj, s a_pj + c a_qj) for every
 *     pair, then columns (a_ip, a_iq) <- (c a_ip - s a_iq, s a_ip + c a_iq) with a_pq = a_qp = 0 set, and the same column
 *     step on Q (disjoint rotations commute).  Ahead of every sweep: if every |a_pq| <= 2^-52 sqrt(a_pp a_qq), p < q, the
 *     iteration ends (status 0); after LNS_ETKF_MAX_SWEEPS = 30 sweeps without that it ends with status 2 and the result
 *     stands as it is.  lam_k = a_kk, taken in ascending order (ties: ascending index) in every sum over k below.
 *         wbar_i = sum_k Q_ik u_k,    u_k = (sum_i Q_ik g_tot_i) / lam_k                (= Q Lambda^-1 Q^T g_tot)
 *         W_ij = ((sum_k (Q_ik f_k) Q_jk) + (sum_k (Q_jk f_k) Q_ik)) / 2,   f_k = sqrt((M - 1) / lam_k)
 *                                                                                        (= sqrt(M-1) Q Lambda^-1/2 Q^T, symmetric)
 *         X_km = W_km + wbar_k
 *     A non-finite entry of S_tot or g_tot: status 1, and X, wbar, lam of THAT sample are NaN; other samples are untouched.
 *     The kernel makes no host read.  With all r = 0: A = dg I, no rotation, X = sqrt((M-1)/dg) I, wbar = 0.
 * 3. Update (per element e of z [B][M][n], double, nothing fused, k ascending):
 *         zbar = (z_0 + ... + z_{M-1}) / M,   Z_k = z_k - zbar,   out_m = (float)(zbar + sum_k Z_k X_km)
 *     (sum: acc = 0; acc = acc + Z_k * X_km).  A thread reads its M values before it writes any, so out may be z; accesses are
 *     scalar: the bits do not depend on alignment.  n = 1 is the update of a per-member param.
 *
 * Not there: localisation, M > 64, additive inflation, correlated observation errors (R is diagonal), observation
 * operators that are not pointwise in the decoded (denormalised) frame.
 *
 * z_in, param, keep_steps_host, B, M, T, mean_out, var_out, z_last: as lns_rollout_latent_ensemble, with 2 <= M <=
 * LNS_ETKF_MAX_MEMBERS.  y_obs [B][n_keep][Cin][Ly][Lx]: the normalised observations of the kept steps (any value where
 * r = 0).  z_analysis [B][M][zper]: the forecast latents of step T - 1 (z_last) updated by X.  Nullable outputs:
 * param_analysis [B][M] (needs param; the per-member param updated by X), X [B][M][M], wbar [B][M], lam [B][M] (ascending),
 * stat [B][n_keep][3] (double), status [B] (int32), mean_out / var_out (lns_rollout_latent_ensemble's bits; var_out needs
 * mean_out), z_last.  The Gram launch follows the decode of each group on its decode stream; the slice sums, the transform and
 * the updates follow the join on the caller's stream.  workspace: lns_rollout_ensemble_analysis_workspace_bytes(B, M, n_keep)
 * = the ensemble layout byte for byte, then one region for the slice partials, S, g, stat, X, wbar, lam, status.
 * Refused before any device work (lns_last_error), in this order: z_in null; y_obs null; rinv null; z_analysis null; a
 * negative stride of rinv; rho < 1 or not finite; B, M, T not positive; M outside 2 .. 64; var_out without mean_out;
 * param_analysis without param; norm of the wrong size; n_keep < 1 and keep_steps as lns_rollout_latent_ensemble; the batch
 * B * M; the model; param. */
#define LNS_ETKF_MAX_MEMBERS 64
int lns_rollout_ensemble_analysis_workspace_bytes(lns_engine* e, int B, int M, int n_keep, size_t* bytes);
int lns_rollout_latent_ensemble_analysis(lns_engine* e, const float* z_in, const float* param, const float* y_obs,
                                         const float* rinv, int64_t rinv_bs, int64_t rinv_ss, int B, int M, int T,
                                         const int* keep_steps_host, int n_keep, const lns_eval_spec* norm /* nullable */,
                                         double rho, float* z_analysis,
                                         float* param_analysis, double* X, double* wbar, double* lam, double* stat,
                                         int32_t* status, float* mean_out, float* var_out, float* z_last, /* all nullable */
                                         void* workspace, size_t workspace_bytes, void* stream);
/* The localised form of this filter, one transform per latent pixel: the next section. */

/* ---- localised ensemble transform Kalman filter: one transform per latent pixel (LETKF) ------------------------------
 * The transform above lies in the span of M - 1 anomaly directions while a latent has hundreds to thousands of degrees of
 * freedom: a sensor in one corner of the plane corrects the latent in the opposite corner through sampling noise alone.
 * The cure is localisation (Hunt, Kostelich, Szunyogh 2007: the LOCAL ETKF), here R-localisation at patch granularity.  The
 * latent of every family is a convolutional [c][h][w] grid over the plane: the decoded frame is cut into the h x w patches of
 * that grid, the Gram sums are taken per patch, the Gram of the local domain of latent pixel l is the Gaspari-Cohn-weighted
 * sum of the patch Grams around it, one Jacobi problem is solved per (sample, latent pixel), and X_l is applied to the c
 * channels of latent pixel l.  A per-member param is not spatial: it is updated by the global transform, taken from the same
 * patch sums with weight 1.  Notation as above; the frame is [C][Ly][Lx], the latent [c][h][w], l = i * w + j.
 *
 * 1. Patches: value p = (ch, y, x) belongs to patch t = ty * w + tx, ty = (y * h) / Ly, tx = (x * w) / Lx in integer arithmetic
 *     (61 x 121 on 7 x 15: patches of 8 or 9 rows and columns).  A patch may be empty (h > Ly); its sums are 0.
 * 2. Patch Gram (per sample b, kept step i and patch t; double): f_m, y, ybar, Y_m, d, w_m = r_p Y_m exactly as in step 1 above,
 *     the one denormalisation device function and the select on r_p > 0 included (unobserved values are not read; NaN there is
 *     harmless).  G_ij (i <= j, G_ji = G_ij), g_i and stat as S_ij, g_i and stat above over the values of the patch: every sum
 *     starts at 0 and takes one fused multiply-add per value of the patch, p ascending (channel, then row, then column); sum r_p:
 *     plain adds.  No slices, no atomics: the result depends on the inputs only.
 * 3. Taper: domain l = (i, j), patch t = (ti, tj): dy = |i - ti|, replaced by min(dy, h - dy) where the y axis is periodic; dx
 *     likewise along x with w.  dist = sqrt((double)(dy*dy + dx*dx)), r = dist / radius, radius the Gaspari-Cohn half-width in
 *     latent pixels (support 2 radius).  With r2 = r r, r3 = r2 r, r4 = r3 r, r5 = r4 r, the terms added from the left in the
 *     order written, nothing fused, the constants 5/3, 5/8, 1/12 each the double quotient:
 *         r <= 1:     rho = (((1 - (5/3) r2) + (5/8) r3) + (1/2) r4) - (1/4) r5
 *         1 < r < 2:  rho = max(0, (((((4 - 5 r) + (5/3) r2) + (5/8) r3) - (1/2) r4) + (1/12) r5) - 2 / (3 r))
 *         r >= 2:     rho = 0
 *     Only + - * / sqrt in IEEE double: a numpy statement of it is held to the bit.
 * 4. Local Gram (per sample and domain; double, nothing fused):
 *         S_l = sum_steps (ascending) sum_t (ascending, rho_lt > 0) rho_lt * G_t,   g_l likewise
 *     as acc = acc + rho * G starting at 0.  S_glob, g_glob: the same sums with rho = 1 over all patches; stat [B][n_keep][3]: per
 *     kept step the sum over all patches, ascending.
 * 5. Transform: step 2 above on (S_l, g_l) for each of the B * h * w domains and once per sample on (S_glob, g_glob) -- the same
 *     kernel, launched with B * h * w blocks (and with B) and n = 1.  Status 1 (a non-finite Gram) marks that domain alone.
 * 6. Update (per sample b, latent pixel l and channel ch, over the M values z_k = z[b][k][ch][l]): zbar, Z_k and
 *         out[b][m][ch][l] = (float)(zbar + sum_k Z_k X_l[k][m])
 *     in the arithmetic and order of step 3 above.  A block reads all it needs before it writes: out may be z.
 *     param_analysis is step 3 above with X_glob.
 * A domain whose support holds no observed value has S_l = 0, hence X_l = sqrt(rho_infl) I and wbar = 0: it keeps its forecast
 * members, apart from inflation.  That is the property that makes the filter local.
 *
 * Not there: M > 64, additive inflation, correlated observation errors, observation operators that are not pointwise in the
 * decoded frame, domains finer or coarser than a latent pixel, a taper other than Gaspari-Cohn, a latent grid above
 * LNS_LETKF_MAX_DOMAINS = 4096 pixels.  The receptive field of the decoder is wider than a patch: the localisation is a
 * modelling choice about which observations may move which latent pixel, not a statement about the decoder.
 *
 * The call: the arguments of lns_rollout_latent_ensemble_analysis plus loc_radius (finite, > 0) and bc_y / bc_x
 * (LNS_FLOW_PERIODIC / LNS_FLOW_WALL: whether the taper's distance wraps along that axis).  Nullable outputs: X_local
 * [B][h*w][M][M], wbar_local and lam_local [B][h*w][M] (double), status_local [B][h*w] (int32); the global X [B][M][M], wbar, lam
 * [B][M], status [B] and stat [B][n_keep][3] of (S_glob, g_glob); param_analysis, mean_out, var_out, z_last as above.  The
 * patch-Gram launch follows the decode of each group on its decode stream; combine, the two transform launches and the updates
 * follow the join on the caller's stream.  No host read, no allocation, no event beyond those of the call above.
 * workspace: lns_rollout_ensemble_analysis_local_workspace_bytes(B, M, n_keep) = the ensemble layout byte for byte, then one
 * region: the patch sums [B][n_keep][h*w][M*M + M + 3] doubles, which dominate it, then S_l, g_l, X_l, wbar_l, lam_l, status_l and
 * the global S, g, stat, X, wbar, lam, status.  A window of a few observed steps is the intended use.
 * Refused before any device work (lns_last_error), in the order of the call above, with two checks directly after the one on
 * rho: "loc_radius must be finite and > 0", then "bc_y / bc_x must be LNS_FLOW_PERIODIC or LNS_FLOW_WALL"; and a latent grid
 * above 4096 pixels after the check of norm. */
#define LNS_LETKF_MAX_DOMAINS 4096
int lns_rollout_ensemble_analysis_local_workspace_bytes(lns_engine* e, int B, int M, int n_keep, size_t* bytes);
int lns_rollout_latent_ensemble_analysis_local(lns_engine* e, const float* z_in, const float* param, const float* y_obs,
                                               const float* rinv, int64_t rinv_bs, int64_t rinv_ss, int B, int M, int T,
                                               const int* keep_steps_host, int n_keep, const lns_eval_spec* norm /* nullable */,
                                               double rho, double loc_radius, int bc_y, int bc_x, float* z_analysis,
                                               double* X_local, double* wbar_local, double* lam_local, int32_t* status_local,
                                               float* param_analysis, double* X, double* wbar, double* lam, double* stat,
                                               int32_t* status, float* mean_out, float* var_out, float* z_last, /* all nullable */
                                               void* workspace, size_t workspace_bytes, void* stream);

/* ---- streaming validation: energy spectra of forecast, truth and error ---------------------------------------------
 * lns_rollout_eval / lns_rollout_latent_eval with, for selected steps, the shell-summed energy spectra of the forecast,
 * of the truth and of their difference, taken where the step is decoded: a spectrum needs the whole plane of a step, i.e.
 * the [B,T,Cin,Ly,Lx] tensor the streaming calls exist to avoid.  A spectrum kernel follows the scoring kernel of a decoded
 * group on its decode stream, one launch per group for the group's selected steps (none selected: no launch), one block
 * per plane.  (No reference counterpart; the ground truth of the tests is numpy.fft in float64.)
 *
 * The statement, for a plane u[y][x] of H x W pixels after the denormalisation D_c of lns_eval_spec (the map written above
 * for lns_rollout_latent_ensemble_eval, product and sum rounded one by one, wall-zero and clamp flags included; eps unused):
 *     F[ky][kx] = sum_y sum_x u[y][x] exp(-2 pi i (ky y / H + kx x / W)),    kx = 0 .. Wh-1, Wh = W/2 + 1  (u is real)
 *     ky' = ky <= H/2 ? ky : ky - H,  kx' = kx,  r2 = ky'*ky' + kx'*kx'
 *     shell(r2) = the integer s with s*(s-1) < r2 <= s*(s+1), 0 for r2 = 0     (round(sqrt(r2)) in integers: no floating tie)
 *     S(H, W) = shell((H/2)^2 + (W/2)^2) + 1 bins (integer division): 24 for 32x32, 92 for 128x128, 108 for 96x192, 68 for 61x121
 *     inv = 1 / (float)(H*W);  a = re * inv;  b = im * inv;  p = w * (a*a + b*b)          (fp32, nothing fused)
 *     w = 1 for kx = 0 and, when W is even, for kx = W/2; else 2 (the conjugate partner, which lies in the same shell)
 *     E[s] = sum of p over the modes of shell s;  by Parseval sum_s E[s] = mean(u^2)
 * Three spectra per plane (b, step, c): row 0 of the forecast P = D_c(yhat), row 1 of the truth Q = D_c(y), row 2 of the
 * error d = P - Q, differenced per pixel in fp32 BEFORE the transform (F_P - F_Q would put the error spectrum's floor at the
 * field's rounding level).  Each of the three fields is transformed directly: the truth is not taken as F_P - F_d.
 *
 * Order of the sums (a function of the plane only; fp32; the contractions are exact-fp32 matrix instructions, i.e. fmaf
 * chains in ascending k starting from +0).  c_N[r] = cospi(2r/N), m_N[r] = -sinpi(2r/N) in fp32 (sincospif), r = (k n) mod N:
 *     row pass     Rre[y][kx] = chain over x = 0 .. W-1 of u[y][x] * c_W[(kx x) mod W];  Rim likewise with m_W
 *     column pass  re[ky][kx] = one chain: y = 0 .. H-1 of c_H[(ky y) mod H] * Rre[y][kx], then y = 0 .. H-1 of (-m_H[.]) * Rim[y][kx]
 *                  im[ky][kx] = one chain: y = 0 .. H-1 of c_H[.] * Rim[y][kx], then y = 0 .. H-1 of m_H[.] * Rre[y][kx]
 *     shell sums   the columns kx are taken in tiles of 32 (kx0 = 0, 32, ...).  In a tile, row ky is cut into runs of
 *                  consecutive kx of equal shell (along a row the shell does not decrease with kx); a run's sum starts
 *                  from 0 and adds its p in ascending kx.  E[s] starts from 0 and adds, tile after tile, within a tile
 *                  in ascending ky = 0 .. H-1 (storage order, not the signed one), the run of shell s of that row, if any.
 * One block owns one plane and stores its 3 x S (1 x S) floats itself: no float atomics, nothing depends on the grouping or
 * the scheduling options, so the streaming calls and lns_op_energy_spectrum (one device function) produce the same bits.
 * A NaN pixel makes every bin of its own plane's spectra that read it NaN and touches no other plane.
 * Bins are index wavenumbers (no physical lengths; on a non-square plane ky and kx count cycles per side).  On the
 * non-periodic families the DFT sees the jump across the walls: those spectra carry its leakage (a k^-2 tail).  Give an
 * axis with walls the basis LNS_SPECTRUM_DCT (below): the DCT-II is the DFT of the plane's mirror extension, which has no
 * jump (measured in float64 on a 96 x 192 ramp in y: 6.8e-3 of the energy at 20 cycles and above under the DFT, 4.0e-7 with
 * a DCT along y).
 *
 * Supported planes: 1 <= H, W <= 192 and H * W <= 18432 (96 x 192); lns_spectrum_bins is host-only and returns S, or
 * LNS_EINVAL for an unsupported plane.
 *
 * A basis per axis.  LNS_SPECTRUM_DFT is everything above (both axes DFT: nothing changes, bit for bit).  An axis of
 * length N with the basis LNS_SPECTRUM_DCT is transformed by a DCT-II:
 *     coefficient index m = 0 .. N-1;  table t_N[r] = cospif((float)r / (float)(2N)) in fp32, read at r = (m (2n + 1)) mod 4N
 *     weight 1 for m = 0, else 2 (no Nyquist exception);  no imaginary part
 * A DFT axis is as above: x keeps kx = 0 .. W/2 with its conjugate weights, y keeps every ky with signed wavenumbers.
 *     row pass     over x ascending, one chain per part: Rre always, Rim only if x is DFT
 *     column pass  over y ascending.  y DCT: re = chain t_H . Rre, im = chain t_H . Rim if Rim exists.
 *                  y DFT: the two-segment chains above, without the Rim terms when Rim does not exist
 *                  (re = chain c_H . Rre, im = chain m_H . Rre)
 *     power        a = re * inv, b = im * inv;  p = (wy * wx) * (a*a + b*b), or (wy * wx) * (a*a) where there is no im
 *                  (fp32, nothing fused; the weights are 1, 2 or 4 and do not round;  wy = 1 on a DFT y axis)
 *     shells       unless both axes are DFT, wavenumbers count HALF cycles per side: a DCT index m counts m, a DFT
 *                  wavenumber k counts 2k; r2 is the sum of the two squares, shell(r2) the integer rule above, so bin s
 *                  lies at s / 2 cycles per side.  S = shell(qy_max^2 + qx_max^2) + 1 with q_max = N - 1 for a DCT axis
 *                  and 2 (N / 2) for a DFT axis.  S for (dft,dft) / (dct-y,dft-x) / (dft-y,dct-x) / (dct,dct):
 *                  24x48: 28 / 54 / 54 / 53;  61x121: 68 / 135 / 135 / 135;  96x192: 108 / 215 / 215 / 214;
 *                  128x128: 92 / 181 / 181 / 181.  The largest S of a supported plane is 215 (one thread per bin).
 *     shell sums   as above: 32-column tiles (a DCT x axis has W columns instead of W/2 + 1), runs of equal shell along a
 *                  row in ascending column (with y DCT and x DFT the shell can rise by two per column: a skipped shell
 *                  has no run in that row), then ascending row in storage order.
 * Parseval holds for every basis: sum_s E[s] = mean(u^2).  Unchanged: the supported planes, the three fields per plane, the
 * error differenced per pixel before the transform, NaN containment, one block per plane, no atomics.
 * lns_spectrum_bins_basis is host-only and returns S, or LNS_EINVAL for an unsupported plane or a basis other than 0 / 1. */
#define LNS_SPECTRUM_DFT 0
#define LNS_SPECTRUM_DCT 1
int lns_spectrum_bins(int H, int W);
int lns_spectrum_bins_basis(int H, int W, int basis_y, int basis_x);

/* lns_rollout_eval / lns_rollout_latent_eval (same arguments, same frame_out / seq_out / frames_out bits, same workspace:
 * lns_rollout_eval_workspace_bytes(B) and nothing more) followed by the spectrum selection: spectrum_steps_host, n_spec >= 1
 * ascending 0-based steps of this call's T (HOST array, read during the call; independent of keep_steps_host), and
 * spectra_out [B][n_spec][Cin][3][S], S = lns_spectrum_bins(Ly, Lx), which every block writes with final values.
 * (With the option "spectrum_basis" set: S = lns_spectrum_bins_basis(Ly, Lx, basis_y, basis_x); the same holds for the
 * spectra of the _stats and _maps entry points.  The entry points are not forked: the basis travels as that option.)
 * Refusals: those of lns_rollout_eval, then (host only, ahead of the batch check) LNS_EINVAL for spectra_out null,
 * n_spec < 1, spectrum_steps_host null / out of range / not ascending, and an unsupported plane.  Trace / timing modes
 * (single stream) and lns_check_finite: as lns_rollout_eval. */
int lns_rollout_eval_spectrum(lns_engine* e, const float* x, const float* param, const float* y_true, int B, int T,
                              const lns_eval_spec* spec, float* frame_out, float* seq_out, const int* keep_steps_host,
                              int n_keep, float* frames_out, void* workspace, size_t workspace_bytes, void* stream,
                              const int* spectrum_steps_host, int n_spec, float* spectra_out);
int lns_rollout_latent_eval_spectrum(lns_engine* e, const float* z_in, const float* param, const float* y_true, int B, int T,
                                     int t0, int T_total, const lns_eval_spec* spec, float* frame_out, float* seq_out,
                                     const int* keep_steps_host, int n_keep, float* frames_out, float* z_last,
                                     void* workspace, size_t workspace_bytes, void* stream,
                                     const int* spectrum_steps_host, int n_spec, float* spectra_out);

/* ---- streaming validation: correlation, gradient error, value statistics and histograms ------------------------------
 * lns_rollout_eval / lns_rollout_latent_eval (and, optionally, the spectra above) with, for selected steps, twelve per-plane
 * statistics of the decoded frame against the truth plane and, optionally, the value histograms of both -- taken where the
 * step is decoded, so the [B,T,Cin,Ly,Lx] rollout is never stored.  A statistics kernel follows the scoring kernel of a decoded
 * group on its decode stream, beside the spectrum launch: one launch per group for the group's selected steps (none
 * selected: no launch), one block of 256 threads per plane.  Reference: training_utils.py:26-32 (pointwise_correlation) and
 * training_utils.py:51-58 (GradientDomainLoss.spatial_fd) followed by relative_lp_loss over (-1, -2); the centred
 * correlation, the moments, the extrema and the histograms have no reference counterpart.
 *
 * The statement, for a plane (b, step, c) of H x W pixels, N = (float)(H*W).  P = D_c(yhat) and Q = D_c(y) are the denormalised
 * forecast and truth, D_c the map of lns_eval_spec as written above for lns_rollout_latent_ensemble_eval (product and sum
 * rounded one by one, wall-zero and clamp flags included).  Everything is fp32, nothing is fused.  Every plane sum is taken
 * in the order of the metric kernels: thread t of 256 adds its terms t, t + 256, ... in ascending order, starting from 0;
 * then the wave sum; then (w0 + w1) + (w2 + w3) over the four waves.  The term index is the row-major pixel index or, for
 * the gradient sums, the row-major index of the difference grid.
 *     pass 1   SP = sum P, SQ = sum Q, PP = sum P*P, QQ = sum Q*Q, PQ = sum P*Q
 *              mP = SP / N, mQ = SQ / N
 *              cos = PQ / ((sqrtf(PP) + eps) * (sqrtf(QQ) + eps))       (pointwise_correlation; eps = spec.eps)
 *              min / max of P and of Q with fminf / fmaxf (a NaN pixel is skipped by them and poisons the sums)
 *     pass 2   a = P - mP, b = Q - mQ;  SA = sum a, SB = sum b, AA = sum a*a, BB = sum b*b, AB = sum a*b
 *              vP = fmaxf((AA - SA*SA/N) / N, 0), vQ likewise, cov = (AB - SA*SB/N) / N     (corrected two-pass, biased)
 *              den = sqrtf(vP) * sqrtf(vQ);  corr = den == 0 ? 0 : cov / den
 *     gradient gyP[y][x] = P[y+2][x] - P[y][x] on (H-2) x W, gxP[y][x] = P[y][x+2] - P[y][x] on H x (W-2); Q likewise
 *              (spatial_fd: no wrap-around, also on the periodic families)
 *              GDy = sum (gyP - gyQ)^2, GGy = sum gyQ^2;  grad_y = sqrtf(GDy / (GGy < eps ? eps : GGy));  x likewise
 *              (H < 3 or W < 3: no terms in either direction, both values are 0)
 * stats_out holds LNS_FIELD_STATS = 12 floats per plane, in this order:
 *     mean_P, mean_Q, var_P, var_Q, corr, cos, grad_y, grad_x, min_P, max_P, min_Q, max_Q
 * (a plane without a non-NaN pixel has min = +inf, max = -inf; in a plane with a NaN pixel the means, cos and the gradient
 * errors of the fields that hold it are NaN, while fmaxf(NaN, 0) = 0 makes its variance 0 and hence corr 0).
 *
 * Histograms are optional and described by lns_stats_spec: nbins in 1 .. 256 and per-channel edges lo_c < hi_c (finite).
 *     scale_c = (float)nbins / (hi_c - lo_c), formed in fp32 on the host (the difference rounded, then the quotient)
 *     v < lo_c: bin 0;  v >= hi_c: bin nbins + 1;  else bin 1 + min(nbins - 1, (int)((v - lo_c) * scale_c))  (two rounded ops)
 *     a NaN is counted nowhere; -inf goes to bin 0, +inf to bin nbins + 1
 * hist_out is int32 [B][n][Cin][2][nbins + 2], row 0 of the forecast, row 1 of the truth.  Counts are taken with integer
 * LDS atomics (order-independent) and stored with ordinary stores.
 * One block owns one plane and stores its 12 floats and its counts itself: no float atomics, no finish kernel, no workspace
 * region; nothing depends on the grouping or the scheduling options, so the streaming calls and lns_op_field_stats (one
 * device function) produce the same bits.  Planes of any size work (the planes are re-read, not staged). */
#define LNS_FIELD_STATS 12
typedef struct lns_stats_spec {
    uint32_t size;      /* sizeof(lns_stats_spec) */
    int32_t nbins;      /* 1 .. 256 */
    float lo[8], hi[8]; /* per channel, in denormalised units */
} lns_stats_spec;

/* lns_rollout_eval_spectrum / lns_rollout_latent_eval_spectrum (same leading arguments; n_spec = 0: no spectra, the three
 * spectrum arguments are ignored) followed by the statistics selection: stats_steps_host, n_stats >= 1 ascending 0-based
 * steps of this call's T (HOST array, read during the call; independent of keep_steps_host and spectrum_steps_host),
 * hspec (nullable), stats_out [B][n_stats][Cin][12] and hist_out (nullable) [B][n_stats][Cin][2][nbins + 2].
 * frame_out / seq_out / frames_out / spectra_out keep the bits of the existing calls; the workspace is
 * lns_rollout_eval_workspace_bytes(B) and nothing more.  Refusals (host only): those of lns_rollout_eval, then those of the
 * spectrum selection when n_spec != 0, then LNS_EINVAL for stats_out null, n_stats < 1, stats_steps_host null / out of
 * range / not ascending, hist_out without hspec, a wrong hspec->size, nbins outside 1 .. 256, a non-finite edge or hi <= lo
 * for a channel below in_channels, and histograms with in_channels > 8.  hspec without hist_out is checked and unused. */
int lns_rollout_eval_stats(lns_engine* e, const float* x, const float* param, const float* y_true, int B, int T,
                           const lns_eval_spec* spec, float* frame_out, float* seq_out, const int* keep_steps_host,
                           int n_keep, float* frames_out, void* workspace, size_t workspace_bytes, void* stream,
                           const int* spectrum_steps_host, int n_spec, float* spectra_out,
                           const int* stats_steps_host, int n_stats, const lns_stats_spec* hspec, float* stats_out,
                           int32_t* hist_out);
int lns_rollout_latent_eval_stats(lns_engine* e, const float* z_in, const float* param, const float* y_true, int B, int T,
                                  int t0, int T_total, const lns_eval_spec* spec, float* frame_out, float* seq_out,
                                  const int* keep_steps_host, int n_keep, float* frames_out, float* z_last,
                                  void* workspace, size_t workspace_bytes, void* stream,
                                  const int* spectrum_steps_host, int n_spec, float* spectra_out,
                                  const int* stats_steps_host, int n_stats, const lns_stats_spec* hspec, float* stats_out,
                                  int32_t* hist_out);

/* ---- streaming validation: per-pixel time-mean, variance, covariance and error maps ---------------------------------
 * Everything above reduces over space, per step.  These maps reduce over time, per pixel: where the error lives, whether
 * the forecast keeps the time-mean state and whether it keeps the temporal variance -- again without storing the
 * [B,T,Cin,Ly,Lx] rollout.  An accumulation kernel follows the statistics launch of a decoded group on its decode stream
 * (one launch per group for the group's selected steps; none selected: no launch) and adds the group's steps to a state of
 * 52 bytes per (b, c, pixel) in the workspace; a finish kernel turns the state into the maps once the horizon is complete.
 * (No reference counterpart: the reference has no per-pixel time statistics.)
 *
 * The statement, for a trajectory b, channel c and pixel p.  P_t = D_c(yhat) and Q_t = D_c(y) are the denormalised fp32
 * forecast and truth of step t, D_c the map of lns_eval_spec as written above for lns_rollout_latent_ensemble_eval (product
 * and sum rounded one by one, wall-zero and clamp flags included).  K = D_c(y_true[b][0][c][p]) is the truth's first frame of
 * the horizon (step 0 of T_total): a per-pixel shift that costs no state and keeps the sums small beside an offset.
 * The selected steps are t >= map_from with (t - map_from) % map_every == 0, in steps of the horizon: a rule, not a list,
 * so a chunked call derives everything from t0, T and T_total and carries no count between calls.  n is their number.
 * In ascending t, all in float64, every operation rounded on its own (no contraction):
 *     a = (double)P_t - (double)K      b = (double)Q_t - (double)K      e = (double)P_t - (double)Q_t
 *     Sa += a   Sb += b   Saa += a*a   Sbb += b*b   Sab += a*b   See += e*e
 *     mx = fmaxf(mx, (float)fabs(e))         (fp32 state, from 0; a NaN is skipped by fmaxf and poisons the sums of that pixel only)
 * The finish, in float64, each result then rounded once to fp32; N = (double)n, d = (double)max(n - 1, 1):
 *     mean_P = K + Sa/N        mean_Q = K + Sb/N
 *     var_P  = v > 0 ? v : 0 with v = (Saa - Sa*Sa/N)/d  (so 0 for a NaN), var_Q likewise     (unbiased; n = 1: exactly 0)
 *     cov    = (Sab - Sa*Sb/N)/d
 *     mse    = See/N           max_err = mx
 * maps_out holds LNS_TIME_MAPS = 7 planes per (b, c), in this order: mean_P, mean_Q, var_P, var_Q, cov, mse, max_err;
 * it is fp32 [B][Cin][7][Ly][Lx].  bias = mean_P - mean_Q, rmse = sqrt(mse) and the temporal correlation
 * cov / sqrt(var_P var_Q) are left to the caller.
 * Why float64 sums and a shift: a sequential fp32 Welford recurrence misses the project's rule max(2e-7, 3 x torch's own fp32
 * error) against float64 (1.4 x the bound at n = 64, 7 to 12 x at n = 1024, orders of magnitude on 1e3 + 1e-2 x); this
 * statement stays near 1e-7 relative for n up to 1024 on unit, 1e-12, 1e12, offset and drifting fields.
 * A thread owns its pixels and is the only writer of their state: no float atomics, no reduction across threads.  The order
 * of a pixel's steps is the only order there is, and it is kept across the decode streams by chaining the accumulation
 * launches with events, so the maps have the same bits for every decode_group / decode_streams / overlap setting, for every
 * chunking of the horizon, and as lns_op_time_maps computes them on the stored rollout (one device function). */
#define LNS_TIME_MAPS 7

/* The optional selections and outputs of a streaming validation call, in one sized struct (the argument lists above do not
 * grow again).  n_spec == 0 / n_stats == 0: none, and the pointers of that part are ignored; otherwise the part is what
 * lns_rollout_eval_spectrum / lns_rollout_eval_stats take, steps relative to this call's T.  map_from / map_every are steps
 * of the horizon (T_total), the same in every chunk. */
typedef struct lns_eval_select {
    uint32_t size;                    /* sizeof(lns_eval_select) */
    int32_t n_spec, n_stats;
    int32_t map_from, map_every;
    int32_t reserved;                 /* 0 */
    const int* spectrum_steps_host;
    float* spectra_out;
    const int* stats_steps_host;
    const lns_stats_spec* hspec;      /* nullable */
    float* stats_out;
    int32_t* hist_out;                /* nullable */
    float* maps_out;                  /* [B][Cin][7][Ly][Lx]; written by the call that completes the horizon */
} lns_eval_select;

/* lns_rollout_eval_workspace_bytes(B), byte for byte, followed by the state region (52 B * Cin * Ly * Lx bytes), rounded to 256. */
int lns_rollout_eval_maps_workspace_bytes(lns_engine* e, int B, size_t* bytes);

/* lns_rollout_eval / lns_rollout_latent_eval (same leading arguments) with the selections of `sel`.  frame_out / seq_out /
 * frames_out / spectra_out / stats_out / hist_out keep the bits of the existing calls.  The call with t0 == 0 clears the state
 * (in stream order), every call adds its selected steps, the call with t0 + T == T_total writes maps_out; until then maps_out
 * is untouched.  The chunks of one horizon share one workspace, which nothing else may use in between.
 * Refusals (host only): those of lns_rollout_eval, of the spectrum selection when n_spec != 0 and of the statistics selection
 * when n_stats != 0; then LNS_EINVAL for sel null or sel->size wrong (the two selections then count as absent), maps_out null,
 * map_every < 1, map_from outside [0, T_total); LNS_ENOMEM for a workspace below lns_rollout_eval_maps_workspace_bytes(B). */
int lns_rollout_eval_maps(lns_engine* e, const float* x, const float* param, const float* y_true, int B, int T,
                          const lns_eval_spec* spec, float* frame_out, float* seq_out, const int* keep_steps_host,
                          int n_keep, float* frames_out, void* workspace, size_t workspace_bytes, void* stream,
                          const lns_eval_select* sel);
int lns_rollout_latent_eval_maps(lns_engine* e, const float* z_in, const float* param, const float* y_true, int B, int T,
                                 int t0, int T_total, const lns_eval_spec* spec, float* frame_out, float* seq_out,
                                 const int* keep_steps_host, int n_keep, float* frames_out, float* z_last,
                                 void* workspace, size_t workspace_bytes, void* stream, const lns_eval_select* sel);

/* ---- error attribution: the rollout error split into the autoencoder's floor and the propagator's drift ------------
 * An LNS model is two separately trained parts.  The validation error of predict does not say which of them to retrain:
 * that needs the reconstruction r_t = D(E(y_t)) of the truth -- the floor no propagator can beat, which the reference scores
 * in the validation loop of every stage-1 script (train_stage1_ns2d.py:104-124, train_stage1_SW.py:107-110,
 * train_stage1_twophase.py:111-114: x_hat = autoencoder(x[:, t]), denormalize, relative_lp_loss(reduce_dim=(-1, -2))) --
 * next to the forecast yhat_t = D(f^t(E(x))) and the truth y_t, pixel by pixel.  These calls form it where the frame is
 * decoded: beside the forecast of a decode group, the truth frames of the group are encoded, the propagated latents are
 * compared with the encoded ones, and the encoded ones are decoded into a second frame buffer.
 *
 * The statement.  For a plane (b, t, c), D_c is the denormalisation of lns_eval_spec (above):
 *     a = D_c(yhat) - D_c(r)      the propagator's error, seen through the decoder
 *     b = D_c(r) - D_c(y)         the autoencoder's error
 *     PP = sum a*a     RR = sum b*b     XX = sum a*b     G = sum D_c(y)^2
 * per_channel = 0: a = (yhat - r) * std and b = (r - y) * std, as the metric forms its error; per_channel = 1: walls and clamp
 * are applied to all three operands before the differences.  PP and XX: fp32, nothing fused, a thread of 256 adds its
 * elements tid, tid + 256, ... ascending from 0, one by one (no float4 grouping: the bits depend on no alignment), then the
 * wave sums and (w0 + w1) + (w2 + w3).  The G of prop and cross: D_c(y) in fp32 (product and sum rounded one by one), its
 * square and the sum in float64 in the same order, rounded to fp32 once.  recon is what lns_metric_rel_l2{,_ch} forms for
 * (r, y) -- the same device function, its own fp32 G: recon holds the bits of lns_metric_rel_l2(D(E(y)), y), as frame holds
 * those of the forecast.  The metric's fp32 G is not reused for prop and cross: on a constant field (1e-12 x under a mean)
 * all its threads round alike, it is 1.9e-7 off, and cross, linear in 1 / g, would miss max(2e-7, 3 x torch's own) by that
 * alone; the two evaluations of the one quantity G differ by fp32 rounding, below what the identity resolves in fp32.
 * Since (a + b) is the forecast's error, D = sum (a+b)^2 = PP + RR + 2 XX in exact arithmetic, and with g = max(G, eps):
 *     frame^2 = prop^2 + recon^2 + cross      prop = sqrtf(PP / g)    recon = sqrtf(RR / g)    cross = (2.0f * XX) / g
 * In exact arithmetic g is one number.  As computed, frame and recon divide by the metric's fp32 evaluation of G, prop and
 * cross by the float64-summed one: two roundings of the same G, a few 1e-7 apart at most, so the identity holds to the fp32
 * rounding of the four sums (tests: 2e-5 of its largest term), not to the bit.
 * cross is signed: whether the propagator's error adds to the autoencoder's (> 0) or compensates it (< 0).
 * The latent drift of (b, t) is latent = sqrtf(sum (z_t - E(y_t))^2 / max(sum E(y_t)^2, eps)) over the whole latent: the bits
 * of lns_metric_rel_l2 on the stored latents viewed as [B][T][1][1][zper] with mean 0, std 1.
 * Every column has a sequence-wise form: the sums are added over t ascending before the ratio, as the metric's finish does.
 * One block writes each slot, no atomics: nothing depends on decode_group / decode_streams / overlap or on the chunking. */
typedef struct lns_eval_attrib {          /* every pointer nullable; at least one set */
    uint32_t size;                        /* sizeof(lns_eval_attrib) */
    float *recon_frame,  *recon_seq;      /* [B,T_total,Cin], [B,Cin] */
    float *prop_frame,   *prop_seq;
    float *cross_frame,  *cross_seq;
    float *latent_frame, *latent_seq;     /* [B,T_total], [B] */
    float *z_true_out;                    /* [B,T_total,zper]: E(y_t) (written by every chunk for its steps) */
    float *recon_frames_out;              /* [B,n_keep,Cin,Ly,Lx]: the reconstructions of keep_steps */
} lns_eval_attrib;

/* lns_rollout_eval_workspace_bytes(B), byte for byte, followed -- each part rounded up to 256 bytes -- by a second frame
 * buffer per decode stream (the size of the first), a true-latent staging buffer [decode_group][B][zper rounded up to 4]
 * floats per decode stream, and three more partial-sum arrays: [B]["eval_max_steps"][Cin][2] (reconstruction),
 * [B]["eval_max_steps"][Cin][3] (PP, XX, G) and [B]["eval_max_steps"][2] (latent). */
int lns_rollout_eval_attrib_workspace_bytes(lns_engine* e, int B, size_t* bytes);

/* lns_rollout_eval / lns_rollout_latent_eval (same leading arguments, same bits in frame_out / seq_out / frames_out) with
 * the outputs of `attrib`.  The frame- and sequence-wise columns are written by the call that completes the horizon
 * (t0 + T == T_total); z_true_out and recon_frames_out by every call for its own steps.  Per decode group the call pays one
 * encoder run per step at batch B (y_true is read in place through its batch stride; param goes to a conditional encoder)
 * and one more decoder run; the truth encode does not depend on the chain and is enqueued ahead of the wait for it.
 * Refusals (host only): those of lns_rollout_eval; then LNS_EINVAL for attrib null or attrib->size wrong, and for an attrib
 * with no output set; LNS_ENOMEM for a workspace below lns_rollout_eval_attrib_workspace_bytes(B), with nothing enqueued.
 * lns_check_finite after these calls: the truth encode and the reconstruction decode run in the decode arenas, where the
 * encoder's and the decoder's records share their bytes, and the last run in every arena is a reconstruction decode.  A
 * non-finite truth frame of the last group of a decode stream therefore shows in that decode's record (through its latent);
 * which plan the message names is not guaranteed, and earlier groups are covered only as "track_nonfinite" covers earlier
 * runs.  No test puts a non-finite truth frame through these calls. */
int lns_rollout_eval_attrib(lns_engine* e, const float* x, const float* param, const float* y_true, int B, int T,
                            const lns_eval_spec* spec, float* frame_out, float* seq_out, const int* keep_steps_host,
                            int n_keep, float* frames_out, const lns_eval_attrib* attrib, void* workspace,
                            size_t workspace_bytes, void* stream);
int lns_rollout_latent_eval_attrib(lns_engine* e, const float* z_in, const float* param, const float* y_true, int B, int T,
                                   int t0, int T_total, const lns_eval_spec* spec, float* frame_out, float* seq_out,
                                   const int* keep_steps_host, int n_keep, float* frames_out, float* z_last,
                                   const lns_eval_attrib* attrib, void* workspace, size_t workspace_bytes, void* stream);

/* Stage-1 validation (the reference loops above): x [B,T,Cin,Ly,Lx] normalised -> frame_out [B,T,Cin], seq_out [B,Cin]
 * (either may be NULL, not both) = lns_metric_rel_l2{,_ch}(autoencoder(x), x), bit for bit, and z_out (nullable)
 * [B,T,zper] = E(x).  Per step: encode, decode into the frame buffer, the metric's group kernel against x itself; the finish
 * kernel at the end; all on the caller's stream.  The reconstruction [B,T,Cin,Ly,Lx] is never stored.  param [B] (one per
 * trajectory) goes to a conditional encoder.  No propagator is needed: LNS_ESTATE only without an autoencoder.  The workspace
 * is the evaluation layout -- lns_rollout_eval_workspace_bytes(B) where that call answers; lns_autoencode_eval_workspace_bytes
 * gives the same number and also serves an engine without propagator.  Refusals as lns_rollout_eval's, in its order. */
int lns_autoencode_eval_workspace_bytes(lns_engine* e, int B, size_t* bytes);
int lns_autoencode_eval(lns_engine* e, const float* x, const float* param, int B, int T, const lns_eval_spec* spec,
                        float* frame_out, float* seq_out, float* z_out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- streaming validation: flow diagnostics (vorticity, divergence, kinetic energy, enstrophy) -----------------------
 * Everything above looks at one channel plane at a time.  Every model family here forecasts a 2-D flow with a velocity pair,
 * and what a flow surrogate is asked first -- does it stay divergence-free like the truth, does it keep the kinetic energy and
 * the enstrophy, how wrong is the vorticity -- needs two channels and their neighbours at once.  These calls take it where
 * the step is decoded, so the [B,T,Cin,Ly,Lx] rollout is never stored: a flow kernel follows the statistics launch of a
 * decoded group on its decode stream (one launch per group for the group's selected steps; none selected: no launch; one
 * block of 256 threads per (b, step)), and a pointwise kernel writes the vorticity of the group's kept steps.
 * (No reference counterpart: the reference has no differential diagnostics.)
 *
 * The statement, for a frame (b, step) of H x W pixels.  P = forecast and Q = truth, each denormalised per pixel by D_c, the
 * map of lns_eval_spec as written above for lns_rollout_latent_ensemble_eval (product and sum rounded one by one, wall-zero
 * and clamp flags included).  U = D_cu(.) and V = D_cv(.) are the two channels lns_flow_spec names; x is the column index, y
 * the row index, both increasing; U is the x-component.  Everything is fp32, nothing is fused.
 * Host constants per axis with spacing d:  rc = (float)(1.0 / (2.0 * (double)d)),  re = (float)(1.0 / (double)d).
 * The derivative of a field f along an axis of length n at index i: the difference rounded first, then the product --
 *     n == 1:                 0.0f
 *     periodic:               (f[(i+1) % n] - f[(i-1+n) % n]) * rc
 *     wall, 0 < i < n-1:      (f[i+1] - f[i-1]) * rc
 *     wall, i == 0:           (f[1] - f[0]) * re
 *     wall, i == n-1:         (f[n-1] - f[n-2]) * re
 * i.e. numpy.gradient(..., edge_order=1) on a wall axis and a wrapped central difference on a periodic one.  A neighbour is
 * D_c of the value at the neighbour's position: a wall-zero channel is zero on the border for the stencil too.
 * Per pixel, one rounded operation per written operator:
 *     w = dxV - dyU   (vorticity)        dv = dxU + dyV   (divergence)        k = U*U + V*V
 * Every plane sum is taken in the order of the metric kernels over the row-major pixel index: thread t of 256 adds its terms
 * t, t + 256, ... in ascending order, starting from 0; then the wave sum; then (w0 + w1) + (w2 + w3) over the four waves.
 *     KP = sum k_P         KQ = sum k_Q         WP = sum w_P*w_P     WQ = sum w_Q*w_Q     DP = sum dv_P*dv_P    DQ = sum dv_Q*dv_Q
 *     WE = sum (w_P-w_Q)^2                      WX = sum w_P*w_Q     VE = sum (a*a + b*b),  a = U_P-U_Q,  b = V_P-V_Q
 * The maxima of fabsf(w_P), fabsf(w_Q) and fabsf(dv_P) are taken with fmaxf, starting from 0 (a NaN pixel is skipped by them
 * and poisons the sums).  Thread 0 finishes in fp32, every op rounded, N = (float)(H*W), eps = spec.eps, and stores
 * LNS_FLOW_STATS = 12 floats per (b, step), in this order:
 *     ke_P = (0.5f*KP)/N        ke_Q = (0.5f*KQ)/N        ens_P = (0.5f*WP)/N       ens_Q = (0.5f*WQ)/N
 *     div_P = sqrtf(DP/N)       div_Q = sqrtf(DQ/N)
 *     vort_err = sqrtf(WE / (WQ < eps ? eps : WQ))
 *     vort_cos = WX / ((sqrtf(WP)+eps) * (sqrtf(WQ)+eps))
 *     vel_err  = sqrtf(VE / (KQ < eps ? eps : KQ))
 *     maxvort_P, maxvort_Q, maxdiv_P
 * The vorticity histogram (the PDF of w) is optional: nbins (0: none, else 1 .. 256) and one edge pair lo < hi in units of w;
 * the bin rule is the one written for the field statistics (scale = (float)nbins / (hi - lo); a NaN is counted nowhere).
 * hist_out is int32 [B][n_flow][2][nbins + 2], row 0 of the forecast, row 1 of the truth; counted with integer LDS atomics,
 * stored with ordinary stores.  vort_frames_out [B][n_keep][Ly][Lx] holds w_P of the keep_steps frames (pointwise; the
 * truth's vorticity comes from lns_op_vorticity on y).
 * One block owns one (b, step) and writes its 12 floats and its counts itself: no float atomics, no finish kernel, no
 * workspace beyond lns_rollout_eval_workspace_bytes(B).  The neighbours are re-read from global memory, so planes of any
 * size work (H * W <= 2^30), axes of length 1 and 2 included.  The result therefore has the same bits for every
 * decode_group / decode_streams / overlap setting, for any chunking of the horizon, and as lns_op_flow_stats /
 * lns_op_vorticity compute it on the stored rollout (one device function). */
#define LNS_FLOW_STATS 12
#define LNS_FLOW_PERIODIC 0
#define LNS_FLOW_WALL 1
typedef struct lns_flow_spec {
    uint32_t size;          /* sizeof(lns_flow_spec) */
    int32_t cu, cv;         /* the channels of the x- and of the y-component */
    int32_t bc_y, bc_x;     /* LNS_FLOW_PERIODIC / LNS_FLOW_WALL per axis */
    float dy, dx;           /* grid spacings, in the units the derivatives are wanted in */
    int32_t nbins;          /* 0: no vorticity histogram, else 1 .. 256 */
    float lo, hi;           /* its edges, in units of the vorticity */
} lns_flow_spec;
typedef struct lns_eval_flow {
    uint32_t size;                    /* sizeof(lns_eval_flow) */
    int32_t n_flow;                   /* >= 1 */
    const int* flow_steps_host;       /* n_flow ascending 0-based steps of this call's T (HOST array, read during the call) */
    const lns_flow_spec* fspec;
    float* flow_out;                  /* [B][n_flow][12] */
    int32_t* hist_out;                /* nullable: [B][n_flow][2][nbins + 2] */
    float* vort_frames_out;           /* nullable: [B][n_keep][Ly][Lx]; needs n_keep > 0 */
} lns_eval_flow;

/* lns_rollout_eval / lns_rollout_latent_eval (same leading arguments) followed by `sel` (nullable: the spectra and the
 * statistics of lns_eval_select, honoured with the bits of their own calls) and `flow`.  frame_out / seq_out / frames_out
 * keep the bits of the existing calls; the workspace is lns_rollout_eval_workspace_bytes(B) and nothing more, which is why
 * a `sel` that asks for time maps (maps_out set, or map_from / map_every not 0) is LNS_EINVAL in this form.
 * Refusals (host only, ahead of the first HIP call), where the time-map form has its own: those of lns_rollout_eval's
 * arguments, of the spectrum selection when n_spec != 0 and of the statistics selection when n_stats != 0; then LNS_EINVAL for
 * a sel of the wrong size (the two selections then count as absent) or one that asks for maps; then for flow null or of the
 * wrong size, flow_out null, n_flow < 1, flow_steps_host null / out of range / not ascending, fspec null or of the wrong size,
 * cu == cv or either outside [0, in_channels), a boundary code other than 0 / 1, dx / dy not finite or <= 0, nbins outside
 * 0 .. 256, a non-finite edge or hi <= lo when nbins > 0, hist_out with nbins == 0, vort_frames_out with n_keep == 0; then
 * lns_rollout_eval's batch, eval_max_steps, model and param refusals. */
int lns_rollout_eval_flow(lns_engine* e, const float* x, const float* param, const float* y_true, int B, int T,
                          const lns_eval_spec* spec, float* frame_out, float* seq_out, const int* keep_steps_host,
                          int n_keep, float* frames_out, void* workspace, size_t workspace_bytes, void* stream,
                          const lns_eval_select* sel /* nullable */, const lns_eval_flow* flow);
int lns_rollout_latent_eval_flow(lns_engine* e, const float* z_in, const float* param, const float* y_true, int B, int T,
                                 int t0, int T_total, const lns_eval_spec* spec, float* frame_out, float* seq_out,
                                 const int* keep_steps_host, int n_keep, float* frames_out, float* z_last,
                                 void* workspace, size_t workspace_bytes, void* stream,
                                 const lns_eval_select* sel /* nullable */, const lns_eval_flow* flow);

/* Post-run health check.  Every kernel of a plan records, per sample, the running maximum of |y| of the tensor it
 * produces (the side channel from which the split-operand convolutions derive their activation scale); a NaN or inf
 * anywhere in a tensor survives in it.  This call synchronises `stream`, reads those few KB back from `workspace`
 * (the one the last lns_encode / lns_decode / lns_propagate / lns_rollout* call for batch B used) and returns
 * LNS_ENONFINITE with lns_last_error() naming the first layer (in execution order) and sample whose output was not
 * finite -- or LNS_OK.  `workspace` / B must be those of the last call (LNS_ESTATE otherwise, also after
 * lns_finalize_weights / lns_set_option, which drop the plans the records belong to; LNS_ENOMEM if workspace_bytes
 * does not cover the records).  Coverage: every tensor a layer wrote in the LAST RUN of each plan of that call,
 * the plan outputs (z, y) included; earlier runs of the same plan in that call (steps < T of a rollout) only with the
 * "track_nonfinite" option.  The reference has no equivalent (its fields would silently carry NaN); nothing on
 * the hot path depends on it. */
int lns_check_finite(lns_engine* e, int B, void* workspace, size_t workspace_bytes, void* stream);

/* ---- training rollout of the latent propagator ------------------------------------------------
 * Reference: LatentDynamics.forward, train_stage2_ns2d.py:126-141 (SW / two-phase: same text) -- z_pred[:, t] =
 * propagator(z_pred[:, t-1]) started at z_in -- feeding loss.backward() at train_stage2_ns2d.py:215.  The loss is the
 * caller's (a Python callable in the reference): lns_train_forward returns z_pred [B,T,c,h,w] and keeps a tape of the
 * step's intermediates in `workspace`; lns_train_backward takes dL/dz_pred and writes the gradient of every propagator
 * parameter (BPTT over the T steps, accumulated in a fixed order: deterministic) and, if asked, of z_in.
 * `params` / `grads`: arrays of lns_num_params() DEVICE pointers indexed like lns_param_info (entries of tensors that
 * do not belong to the propagator are ignored and may be null); parameters are read from the device at every call
 * (an optimiser updates them in place between calls) -- lns_set_weight / lns_finalize_weights are not involved.
 * All contractions run on the exact-fp32 matrix instruction.  Plain propagators (NS2d, SW, two-phase) and the
 * conditional one (train_stage2_twophase_conditional.py:25-121; `param` [B]; its gradient: lns_train_backward_ex).  The same
 * workspace and parameter values must be used for the backward call.
 * lns_train_workspace_bytes needs no device for the size; when the process has one it also builds the shape's plan (device
 * index maps) on the caller's current device, so that the first run call does not.
 * Option "train_wgrad" = 1 appends one area to the layout (everything before it keeps its offset): the partial sums of the
 * plan's largest weight-gradient launch, S * Cout * Cin * k * k floats rounded up to 64 floats, where S is
 * lns_op_conv_wgrad_scratch_bytes' slice count for (B, Cin, Cout, h, w, k).  With the option at 0 the sizes are what they
 * were without it.  A workspace sized under 0 and used under 1 is refused with LNS_ENOMEM (the message names the needed
 * size) before anything is enqueued. */
int lns_train_workspace_bytes(lns_engine* e, int B, int h, int w, int T, size_t* bytes);
int lns_train_forward(lns_engine* e, const float* const* params, const float* z_in, const float* param_or_null,
                      int B, int h, int w, int T, float* z_pred, void* workspace, size_t workspace_bytes, void* stream);
int lns_train_backward(lns_engine* e, const float* const* params, const float* z_in, const float* z_pred,
                       const float* grad_z_pred, int B, int h, int w, int T, float* const* grads, float* grad_z_in,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ---- device-resident training step: loss, backward through time and Adam ---------------------------------------
 * Reference: the body of the stage-2 training loop, train_stage2_ns2d.py:210-216 (same text in train_stage2_SW.py and
 * train_stage2_twophase*.py):
 *     optim.zero_grad(); loss = model(z_in, z_out[, param], F.smooth_l1_loss); loss.backward(); optim.step()
 * with optim = torch.optim.Adam(propagator parameters) (:179).  The calls below only enqueue kernels on `stream`: no
 * host synchronisation, no device allocation and no copy from host memory (the first call for a shape builds the
 * training plan, as lns_train_forward does).  Their argument errors (LNS_EINVAL / LNS_ESTATE / LNS_ENOMEM, named by the
 * error message) are decided before any device work.
 *
 * F.smooth_l1_loss(pred, target, reduction='mean', beta) (train_stage2_ns2d.py:213) and its gradient in one pass:
 *     d = pred - target;  l = 0.5 d^2 / beta if |d| < beta else |d| - 0.5 beta;  *loss_out = mean(l)   (device float)
 *     grad_out (nullable, n floats) = dL/dpred = (d / beta if |d| < beta else sign(d)) / n
 * scratch: device, scratch_floats >= ceil(n / LNS_SL1_CHUNK) floats of block partial sums.  The sums are combined in a
 * fixed order that does not depend on the launch: the loss is bit-reproducible.  beta > 0 (torch's beta = 0 is L1: use
 * another kernel), 1 <= n <= LNS_SL1_CHUNK * 2^30 (LNS_EINVAL otherwise).  No engine: the message of a refused call is lns_create_error()'s (this thread). */
#define LNS_SL1_CHUNK 4096
int lns_loss_smooth_l1(const float* pred, const float* target, int64_t n, float beta, float* loss_out, float* grad_out,
                       float* scratch, size_t scratch_floats, void* stream);

/* torch.optim.Adam.step() (train_stage2_ns2d.py:216; no amsgrad, not maximize; L2 weight_decay added to the gradient):
 *     g' = g + weight_decay p;  m = beta1 m + (1 - beta1) g';  v = beta2 v + (1 - beta2) g'^2
 *     p -= lr / (1 - beta1^step) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
 * of many tensors in one launch (the pointer table travels in the kernel-argument block: 96 tensors per launch).
 * `step` is the 1-based count of THIS update; it lives on the host, the bias corrections are computed there in double.
 * size = sizeof(lns_adam_spec): another value is LNS_EINVAL, as are lr < 0, betas outside [0, 1), eps <= 0,
 * weight_decay < 0 and step < 1. */
typedef struct lns_adam_spec {
    uint32_t size;
    uint32_t reserved;                          /* 0 */
    double lr, beta1, beta2, eps, weight_decay; /* doubles, as torch keeps them: 1 - beta2 formed from a float beta2 is off by 1e-5 */
    int64_t step;
} lns_adam_spec;
/* params / grads / exp_avg / exp_avg_sq: arrays of lns_num_params() DEVICE pointers indexed like lns_param_info (any
 * tensor of the table, not only the propagator's); an entry is updated when all four are non-null and left untouched
 * otherwise.  Runs on the caller's current device. */
int lns_adam_step(lns_engine* e, float* const* params, const float* const* grads, float* const* exp_avg,
                  float* const* exp_avg_sq, const lns_adam_spec* spec, void* stream);
/* The same for any n fp32 tensors of numel[i] elements (0 < numel < 2^31): the optimiser of lns_amd/optim.py.  No engine:
 * the message of a refused call is lns_create_error()'s. */
int lns_adam_step_tensors(int n, float* const* params, const float* const* grads, float* const* exp_avg,
                          float* const* exp_avg_sq, const int64_t* numel, const lns_adam_spec* spec, void* stream);

/* The whole step: lns_train_forward -> smooth-L1 loss and dL/dz_pred -> lns_train_backward -> Adam, enqueued on `stream`
 * in that order.  z_in [B,1,c,h,w] (= [B,c,h,w]), z_out [B,T,c,h,w]: the pre-encoded targets as the reference's loader
 * yields them; params / grads / exp_avg / exp_avg_sq as above.  `grads` are the caller's buffers and hold this step's
 * gradients afterwards (to clip or log); *loss_out (device float) is the loss BEFORE the update, like `loss` in the
 * reference loop.  adam_spec == NULL: loss and gradients only (exp_avg / exp_avg_sq are ignored).  With adam_spec every
 * propagator parameter needs all four pointers (LNS_EINVAL otherwise).  LNS_ESTATE: the engine has no propagator;
 * (both calls);
 * LNS_ENOMEM: workspace smaller than lns_train_step_workspace_bytes, which is lns_train_workspace_bytes followed by
 * z_pred, dL/dz_pred (B*T*c*h*w floats each) and the loss partials, each rounded up to 256 bytes.  Noise injection
 * (z_in + randn * noise_level, train_stage2_ns2d.py:211-212) stays the caller's. */
int lns_train_step_workspace_bytes(lns_engine* e, int B, int h, int w, int T, size_t* bytes);
int lns_train_step(lns_engine* e, float* const* params, const float* z_in, const float* z_out, const float* param_or_null,
                   int B, int h, int w, int T, float beta, float* const* grads, float* const* exp_avg,
                   float* const* exp_avg_sq, const lns_adam_spec* adam_spec, float* loss_out, void* workspace,
                   size_t workspace_bytes, void* stream);

/* ---- gradient-norm clipping and AdamW in the training step ----------------------------------------------------------
 * No reference counterpart: the reference's loop (train_stage2_ns2d.py:210-216) neither clips nor decays.  What is
 * reproduced is torch's own text: torch.nn.utils.clip_grad_norm_(parameters, max_norm) (norm_type = 2)
 *     norm = || all gradients ||_2;  coef = min(1, max_norm / (norm + 1e-6));  g *= coef
 * and torch.optim.AdamW (p *= 1 - lr weight_decay, then Adam on the gradient alone).  Everything is enqueued on `stream`:
 * no host read-back, no allocation, no copy from host memory; argument errors are decided before any device work.
 *
 * The norm: a block squares and sums LNS_NORM_CHUNK consecutive elements of one tensor in double (the square of an fp32
 * value is exact there) and stores one double partial; one finishing block adds the partials in ascending order.  No
 * atomics; the order depends on the tensors' lengths alone, so the norm is bit-reproducible.  *norm_out = (float)sqrt(sum);
 * *coef_out as above in fp32 (max_norm <= 0: the norm is computed and coef = 1; a NaN norm gives a NaN coef, as torch).
 * flags: an lns_update_spec's (unknown bits: LNS_EINVAL; LNS_UPDATE_DECOUPLED_WD means nothing here).  With
 * LNS_UPDATE_SKIP_NONFINITE a norm that is inf or NaN writes coef = -1 -- the one negative value, which the
 * update and scale calls below read as "change nothing" -- and adds 1 to *skipped_counter (device uint32, nullable; the
 * caller zeroes it once).  scratch: device, lns_grad_norm_scratch_bytes = 8 * sum(ceil(numel[i] / LNS_NORM_CHUNK)) rounded
 * up to 256 (host only; over all n entries).  0 < numel[i] < 2^31; entries whose gradient pointer is null are left out.
 * norm_out / coef_out: device floats, either may be null.  LNS_ENOMEM: scratch null or short.  No engine: the message of a
 * refused call is lns_create_error()'s. */
#define LNS_NORM_CHUNK 2048
#define LNS_UPDATE_DECOUPLED_WD 1u     /* weight_decay is AdamW's: p *= 1 - lr weight_decay, nothing added to the gradient */
#define LNS_UPDATE_SKIP_NONFINITE 2u   /* a non-finite gradient norm skips the update (see above) */
int lns_grad_norm_scratch_bytes(int n, const int64_t* numel, size_t* bytes);
int lns_grad_norm_tensors(int n, const float* const* grads, const int64_t* numel, double max_norm, float* norm_out,
                          float* coef_out, uint32_t* skipped_counter, uint32_t flags, void* scratch, size_t scratch_bytes,
                          void* stream);
/* g *= *coef for every tensor (the second half of clip_grad_norm_ when no update follows); coef == -1: nothing. */
int lns_grad_scale_tensors(int n, float* const* grads, const int64_t* numel, const float* coef, void* stream);

/* lns_adam_spec plus what the clipped step needs.  size = sizeof(lns_update_spec); unknown flag bits and a NaN max_norm
 * are LNS_EINVAL like a wrong size (the message names the field); lr .. step are checked as in lns_adam_spec.
 * max_norm <= 0: the norm is computed, nothing is clipped.  (lns_update_step_tensors takes its coefficient from the caller
 * and does not read max_norm.) */
typedef struct lns_update_spec {
    uint32_t size;
    uint32_t flags;                             /* LNS_UPDATE_* */
    double lr, beta1, beta2, eps, weight_decay;
    int64_t step;
    double max_norm;
} lns_update_spec;
/* Adam / AdamW of n tensors on g * *coef, in one launch per 96 tensors.  coef (device float, nullable): with it the
 * gradient buffers hold g * coef afterwards, as .grad does after clip_grad_norm_; null: gradients are used and left as
 * they are.  *coef == -1 (a skipped step): params, exp_avg, exp_avg_sq and grads keep their bits.  `step` lives on the host
 * and cannot know about a skip: the caller advances it all the same, so a skipped step still moves the bias corrections on. */
int lns_update_step_tensors(int n, float* const* params, float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                            const int64_t* numel, const lns_update_spec* spec, const float* coef, void* stream);

/* lns_train_step with the clipped update: forward -> loss -> backward -> norm of the propagator's gradients -> update, in
 * that order on `stream`; honours "train_wgrad" like lns_train_step.  `spec` is required (gradients alone: lns_train_step
 * with adam_spec == NULL).  *norm_out (device float, nullable) = the norm before clipping; `grads` hold the clipped
 * gradients afterwards.  The workspace is lns_train_step's followed by the norm partials (8 bytes per LNS_NORM_CHUNK of
 * every propagator tensor), the coefficient (float), the norm (float; used when norm_out is null) and the counter of
 * skipped steps (uint32), each rounded up to 256 bytes: the coefficient sits 768 bytes, the counter 256 bytes before the
 * end of lns_train_step_clip_workspace_bytes.  The caller zeroes the counter once after allocating.  Errors as
 * lns_train_step. */
int lns_train_step_clip_workspace_bytes(lns_engine* e, int B, int h, int w, int T, size_t* bytes);
int lns_train_step_clip(lns_engine* e, float* const* params, const float* z_in, const float* z_out, const float* param_or_null,
                        int B, int h, int w, int T, float beta, float* const* grads, float* const* exp_avg,
                        float* const* exp_avg_sq, const lns_update_spec* spec, float* loss_out, float* norm_out,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ---- latent fit: the rollout run backwards onto data -----------------------------------------------------------------
 * No reference counterpart: the reference trains the propagator and never differentiates with respect to its inputs.
 * Which initial latent makes the rollout agree with several observed frames, and which `param` explains an observed
 * sequence, are answered by descending on z0 [B,c,h,w] and / or param [B] with the propagator's weights held fixed.
 *
 * lns_train_backward_ex = lns_train_backward (same arguments, same launches, same bits) with two additions:
 *   * grads == NULL selects the STATE-ONLY ADJOINT: no weight-gradient, bias-gradient or GroupNorm-affine launch and no
 *     parameter output of the conditional vector network (their kernels take null outputs; nothing is written anywhere in
 *     their place), and the copy that only feeds the one-block-per-tile in_proj weight gradient is skipped.  The data path
 *     is the same kernels in the same order: grad_z_in has the bits of the full call.  The workspace only has to cover the
 *     layout WITHOUT the partial-sum area of "train_wgrad" = 1 (which is appended), so one sized under either value is
 *     accepted.  lns_train_backward itself still refuses grads == NULL.
 *   * grad_param [B] (nullable; both modes): d loss / d param of the conditional propagator (LNS_EINVAL on a plain one).
 *     The chain: the per-block d m and d emb sums and the vector network's backward as they are, d ce summed over the
 *     blocks, then d fe = W0^T d l0 and
 *         grad_param[b] = sum_k f_k (-sin(a_k) dfe[b,k] + cos(a_k) dfe[b,half+k]),  a_k = param[b] f_k,
 *     f_k = exp(-ln(1e4) k / half) as the forward forms it, summed in ascending k by one thread per sample in fp32; the
 *     zero column of an odd embedding width is not read.  cos(a_k) and sin(a_k) are the forward's own fe, which the
 *     workspace still holds: the call takes no `param`. */
int lns_train_backward_ex(lns_engine* e, const float* const* params, const float* z_in, const float* z_pred,
                          const float* grad_z_pred, int B, int h, int w, int T, float* const* grads_or_null, float* grad_z_in,
                          void* workspace, size_t workspace_bytes, void* stream, float* grad_param_or_null);

/* Observation loss of a rollout and its gradient, one loss per trajectory (each sample is its own inverse problem).
 * z_pred [B,T,n] (n = c*h*w), obs [B,n_obs,n]; HOST arrays obs_steps[n_obs] (0-based indices into the T axis, strictly
 * ascending, each < T) and obs_weight[n_obs] (finite, >= 0; NULL: all 1); 1 <= n_obs <= LNS_OBS_MAX (the table travels
 * in the kernel-argument block).  z0 and z_background [B,n] come together or not at all: the background term
 * `background` (lambda >= 0) * mean_i (z0 - z_background)_i^2.
 *     per  [B,n_obs] (nullable)  m_bk = (1/n) sum_i d_i^2,  d_i = z_pred[b,t_k,i] - obs[b,k,i]
 *     loss [B]                   sum_k w_k m_bk + lambda (1/n) sum_i (z0 - z_b)_i^2
 *     grad_z_pred [B,T,n]        (float)(2 w_k / n) * d_i on observed steps, exact zeros on every other step whatever the
 *                                buffer held
 *     grad_z0_bg [B,n] (nullable, needs z0)   (float)(2 lambda / n) * (z0 - z_b)_i
 * Order: d in fp32; its square and every sum in double.  One 256-thread block per (b, t) plane: a thread adds its
 * elements i = tid, tid + 256, ... in ascending order, the 64 lanes of a wave are summed as a balanced butterfly
 * (neighbours first), the four waves as (w0 + w1) + (w2 + w3).  A finishing launch, one thread per sample, forms m_bk =
 * sum * (1/n), adds w_k m_bk in ascending k and the background term last, all in double, and rounds once.  No atomics:
 * bit-reproducible.  The coefficients 2 w_k / n and 2 lambda / n are rounded once on the host from double; the gradient is
 * one fp32 subtraction and one fp32 multiplication per element, not contracted.  Scalar accesses: the bits do not depend
 * on the alignment of the pointers.  scratch: device, lns_loss_obs_mse_scratch_bytes = 8 * B * (n_obs + 1) rounded up to
 * 256 (LNS_ENOMEM when null or short).  No engine: the message of a refused call is lns_create_error()'s. */
#define LNS_OBS_MAX 64
int lns_loss_obs_mse_scratch_bytes(int B, int n_obs, size_t* bytes);
int lns_loss_obs_mse(const float* z_pred, const float* obs, int B, int T, int64_t n, int n_obs, const int* obs_steps_host,
                     const double* obs_weight_host_or_null, const float* z0_or_null, const float* z_background_or_null,
                     double background, float* per_or_null, float* loss, float* grad_z_pred, float* grad_z0_bg_or_null,
                     void* scratch, size_t scratch_bytes, void* stream);

/* One iteration of the fit, enqueued on `stream` in this order:
 *     lns_train_forward over T = obs_steps[n_obs-1] + 1 steps from z0 -> lns_loss_obs_mse -> the state-only
 *     lns_train_backward_ex -> g_z = grad_z_in + grad_z0_bg (a separate fp32 add, only with z_background) ->
 *     lns_update_step_tensors on z0 (spec.state) and on param (spec.param), one launch each, coef == NULL
 * -- the bits of those calls made one after the other.  flags: LNS_FIT_STATE and / or LNS_FIT_PARAM (neither, or another
 * bit: LNS_EINVAL; LNS_FIT_PARAM on a plain propagator: LNS_EINVAL).  z0 [B,c,h,w] and param [B] are updated IN PLACE when
 * fitted and only read otherwise (param: required by the conditional propagator, ignored by the plain one).  obs
 * [B,n_obs,c,h,w]; z_background [B,c,h,w] or NULL (no background term; background > 0 without it is LNS_EINVAL; the term
 * enters the loss whenever it is given and the gradient when the state is fitted).  obs_steps (each < 2^24) / obs_weight as
 * in lns_loss_obs_mse.
 * state / param: an lns_update_spec each (own learning rate and step count); their flags and max_norm must be 0
 * (LNS_EINVAL naming the field: there is no norm pass inside the step).  g_z / exp_avg_z / exp_avg_sq_z [B,c,h,w] and g_p /
 * exp_avg_p / exp_avg_sq_p [B]: the caller's, required for what is fitted; the gradients stay in g_z / g_p.  loss [B]: the
 * loss BEFORE the update; per [B,n_obs] nullable.  As in lns_train_step: no host synchronisation, no allocation, no copy
 * from host memory, every refusal decided before the first HIP call.
 * Workspace (lns_fit_step_workspace_bytes(e, B, h, w, T, n_obs); LNS_ENOMEM names the needed size): lns_train_step_
 * workspace_bytes' layout for T steps | the double partials, 8 * B * (n_obs + 1) bytes | grad_z0_bg, 4 * B * c * h * w
 * bytes -- each part rounded up to 256 bytes. */
#define LNS_FIT_STATE 1u
#define LNS_FIT_PARAM 2u
typedef struct lns_fit_spec {
    uint32_t size;                              /* sizeof(lns_fit_spec) */
    uint32_t flags;                             /* LNS_FIT_* */
    int32_t n_obs;
    int32_t reserved;                           /* 0 */
    const int* obs_steps;                       /* host, n_obs entries */
    const double* obs_weight;                   /* host, n_obs entries, or NULL */
    double background;                          /* lambda */
    lns_update_spec state, param;
} lns_fit_spec;
int lns_fit_step_workspace_bytes(lns_engine* e, int B, int h, int w, int T, int n_obs, size_t* bytes);
int lns_fit_step(lns_engine* e, const float* const* params, float* z0, float* param_or_null, const float* obs,
                 const float* z_background_or_null, int B, int h, int w, const lns_fit_spec* spec, float* g_z,
                 float* exp_avg_z, float* exp_avg_sq_z, float* g_p, float* exp_avg_p, float* exp_avg_sq_p, float* loss,
                 float* per_or_null, void* workspace, size_t workspace_bytes, void* stream);

/* ---- latent fit: Gauss-Newton ("fit_gauss_newton" in lns_build_has) ------------------------------------------------------
 * The fit of z0 is a nonlinear least-squares problem, and both halves of its Gauss-Newton operator are calls of this
 * header: lns_train_tangent gives J v, the state-only lns_train_backward_ex gives J^T w.  Per sample b, n = c*h*w,
 * J_k = d z_pred[t_k] / d z0 at the current z0:
 *     L(z0)   = sum_k w_k (1/n) |z_pred[t_k] - obs_k|^2 + lambda (1/n) |z0 - z_b|^2          (lns_loss_obs_mse's loss)
 *     H v     = sum_k (2 w_k / n) J_k^T (J_k v) + (2 lambda / n + mu) v                       (mu >= 0: Levenberg damping, absolute)
 *     v^T H v = sum_k (2 w_k / n) |J_k v|^2 + (2 lambda / n + mu) |v|^2
 * An outer iteration solves H delta = -g (g: the gradient lns_fit_step forms in g_z) by n_cg steps of conjugate gradients
 * from delta = 0 and adds delta to z0.  No reference counterpart.
 *
 * lns_train_gn_product follows an lns_train_forward(..., T, ...) from z_in on the SAME workspace with the SAME params, as
 * lns_train_tangent does, and enqueues: a copy of v [B,c,h,w] into the workspace's latent tangent (v is only read) ->
 * lns_train_tangent (K = 1, steps 0 .. T - 1, jv_out = the cotangent area) -> the weighting, in place on that area: on the
 * plane of observed step t_k the double sum of squares of the unscaled values, then jv = (float)(2 w_k / n) * jv (the
 * coefficient of lns_loss_obs_mse); exact zeros on every other step; and the double sum of v^2 -> the state-only
 * lns_train_backward_ex with that area as grad_z_pred into hv [B,c,h,w] (not v) -> vhv [B] DOUBLE (nullable):
 * sum_k (2 w_k / n) |J_k v|^2 in ascending k, then + (2 lambda / n + mu) |v|^2, one thread per sample, all in double
 * (2 w_k / n and 2 lambda / n + mu formed in double on the host); and, when c_d = (float)(2 lambda / n + mu) != 0,
 * hv = hv + c_d * v, one fp32 multiplication and one fp32 addition per element, not contracted.  vhv comes from the
 * tangent side alone: a sum of squares, never negative, whatever rounding the adjoint adds to hv.
 * Order of the sums: lns_loss_obs_mse's (256-thread block per plane, a thread adds i = tid, tid + 256, ... ascending in
 * double, the wave as a butterfly with neighbours first, the four waves (w0 + w1) + (w2 + w3)).  No atomics; scalar
 * accesses; bit-reproducible; the tape and the forward weight packs are left as they were, so further products and
 * lns_train_tangent calls may follow on the same forward.
 * T must equal obs_steps[n_obs-1] + 1 (LNS_EINVAL otherwise): the cotangent then has exactly grad_z_pred's layout.
 * Workspace (lns_train_gn_product_workspace_bytes(e, B, h, w, T, n_obs); needs no GPU; the forward must be given it):
 * lns_train_tangent_workspace_bytes(e, B, h, w, T, 1)'s layout, no offset moved | the cotangent, 4 * B * T * n bytes | the
 * double partials, 8 * B * (n_obs + 1) bytes -- each part rounded up to 256 bytes.
 * Refusals, decided on the host in this order before anything is enqueued: null e / params / z_in / z_pred / v / hv, hv == v
 * (size query: null bytes, then no propagator, B, T, n_obs, the latent size); no propagator (LNS_ESTATE); B < 1 or beyond the
 * batch limit; the latent size; B * n >= 2^31; the observation table as in lns_loss_obs_mse (n_obs, steps, weights,
 * background); T != last step + 1; damping negative or not finite; a null propagator parameter pointer; workspace null or
 * short (LNS_ENOMEM naming the bytes); then the pointers' device.  A refused call touches nothing.  No host
 * synchronisation, allocation or host copy inside the call. */
int lns_train_gn_product_workspace_bytes(lns_engine* e, int B, int h, int w, int T, int n_obs, size_t* bytes);
int lns_train_gn_product(lns_engine* e, const float* const* params, const float* z_in, const float* z_pred, int B, int h,
                         int w, int T, int n_obs, const int* obs_steps_host, const double* obs_weight_host_or_null,
                         double background, double damping, const float* v, float* hv, double* vhv_or_null,
                         void* workspace, size_t workspace_bytes, void* stream);

/* Conjugate gradients per sample on fp32 vectors [B,n] with every scalar in double on the device (rs, rs0 [B] double).
 *   lns_op_cg_start:  x = 0, r_i = -g_i, p = r, rs[b] = rs0[b] = sum_i (double)r_i^2.
 *   lns_op_cg_update: one step with hp = H p.  php [B] double: the caller's <p, H p>; NULL: sum_i (double)p_i (double)hp_i here.
 *       active = isfinite(rs) && rs > 0 && isfinite(php) && php > 0 && rs > tol^2 rs0
 *       not active: NOTHING of this sample is written (x, r, p, rs keep their bits, applied[b] is not incremented: a frozen
 *                   sample never receives a NaN)
 *       alpha = rs / php;  x_i = (float)((double)x_i + alpha (double)p_i);  r_i = (float)((double)r_i - alpha (double)hp_i)
 *       rs' = sum_i (double)r_i^2 (the new r);  beta = rs' / rs;  p_i = (float)((double)r_i + beta (double)p_i);  rs = rs'
 *       applied[b] += 1   (int32 [B], nullable; the caller zeroes it)
 * Every product and sum in double, each element rounded once, nothing contracted; one 256-thread block per sample, the
 * sums in lns_op_orthonormalize's order.  Scalar accesses: the bits do not depend on the pointers' alignment.  Refuse null
 * required pointers, B outside 1 .. 65535, n outside 1 .. 2^31 - 1, tol negative or not finite (LNS_EINVAL; message:
 * lns_create_error()); never synchronise. */
int lns_op_cg_start(const float* g, float* x, float* r, float* p, int B, int64_t n, double* rs, double* rs0, void* stream);
int lns_op_cg_update(float* x, float* r, float* p, const float* hp, const double* php_or_null, int B, int64_t n, double tol,
                     double* rs, const double* rs0, int32_t* applied_or_null, void* stream);

/* One outer Gauss-Newton iteration on z0 [B,c,h,w] (updated IN PLACE), enqueued on `stream` in this order:
 *     lns_train_forward over T = obs_steps[n_obs-1] + 1 steps -> lns_loss_obs_mse -> the state-only lns_train_backward_ex ->
 *     g = grad_z_in + grad_z0_bg (a separate fp32 add, only with z_background) -> lns_op_cg_start ->
 *     n_cg x ( lns_train_gn_product on the direction p, then lns_op_cg_update with php = the product's vhv ) ->
 *     z0 = z0 + x (a plain fp32 add)
 * -- the bits of those calls made one after the other; up to the add that forms g it is lns_fit_step's first half, so for
 * the same z0 loss [B] (the loss BEFORE the update) and per [B,n_obs] (nullable) have lns_fit_step's bits.  cg_resid [B]
 * float (nullable): (float)sqrt(rs / rs0) after the last step, 0 where the gradient is 0; applied [B] int32 (nullable): the
 * steps that were applied to each sample (zeroed here).  `param` [B] is a known input of the conditional propagator --
 * required there, ignored on the plain one, never fitted: the tangent has no param direction.  z_background / background as
 * in lns_fit_step.  spec: flags must be 0, 1 <= n_cg <= LNS_GN_CG_MAX, damping (mu) and cg_tol finite and >= 0.
 * Workspace (lns_fit_gn_step_workspace_bytes(e, B, h, w, T, n_obs); LNS_ENOMEM names the needed size):
 * lns_train_gn_product_workspace_bytes' layout | z_pred, 4 * B * T * n bytes | grad_z0_bg | g | x | r | p | hp, 4 * B * n
 * bytes each | rs | rs0 | vhv, 8 * B bytes each -- each part rounded up to 256 bytes.
 * Refusals, decided on the host in this order before anything is enqueued: null e; no propagator (LNS_ESTATE); spec null or
 * of another size; flags; n_cg; cg_tol; null params, z0 / obs, param (conditional), loss; background > 0 without
 * z_background; then lns_train_gn_product's from "B < 1" on (T follows the table); workspace null or short (LNS_ENOMEM);
 * then the pointers' device.  A refused call touches nothing.  No host synchronisation, allocation or host copy. */
#define LNS_GN_CG_MAX 64
typedef struct lns_gn_spec {
    uint32_t size;                              /* sizeof(lns_gn_spec) */
    uint32_t flags;                             /* 0 */
    int32_t n_obs;
    int32_t n_cg;                               /* 1 .. LNS_GN_CG_MAX */
    const int* obs_steps;                       /* host, n_obs entries */
    const double* obs_weight;                   /* host, n_obs entries, or NULL */
    double background;                          /* lambda */
    double damping;                             /* mu */
    double cg_tol;                              /* a sample stops when |r| <= cg_tol |r0| */
} lns_gn_spec;
int lns_fit_gn_step_workspace_bytes(lns_engine* e, int B, int h, int w, int T, int n_obs, size_t* bytes);
int lns_fit_gn_step(lns_engine* e, const float* const* params, float* z0, const float* param_or_null, const float* obs,
                    const float* z_background_or_null, int B, int h, int w, const lns_gn_spec* spec, float* loss,
                    float* per_or_null, float* cg_resid_or_null, int32_t* applied_or_null, void* workspace,
                    size_t workspace_bytes, void* stream);

/* ---- tangent-linear rollout: perturbations carried forward along a trajectory -----------------------------------------
 * No reference counterpart: the reference never linearises its propagator.  lns_train_backward_ex with no gradient array
 * carries a cotangent back through the rollout, J^T w; this is the other half of the pair, J v, so that
 * <J v, w> = <v, J^T w> holds between the two calls.
 *
 * lns_train_tangent follows an lns_train_forward(..., T, ...) on the SAME workspace with the SAME params and reads that
 * call's tape and forward weight packs.  v [B,K,c,h,w] holds K tangents of every sample's latent BEFORE step t0; the call
 * advances them through the steps t0 .. t0 + nsteps - 1 of the taped trajectory, in place (v <- J_t v per step, J_t the
 * Jacobian of propagator step t with respect to its input latent, at the tape's point), and with jv_out
 * [B,K,nsteps,c,h,w] also stores them after every one of those steps (its last step is v's new value, bit for bit).  It
 * takes neither z_in nor param: the tape has what they gave, and the conditional propagator's emb and m depend on param
 * only, so their tangents are zero (dh = conv1.3(da1) with no broadcast add, dxm = dx1 (1 + m)).
 * Per step, lns_train_forward's text line by line: every convolution is the forward launch without bias on the plan of
 * batch B*K (K tangents ride the batch axis; row r = b*K + k reads the tape of sample b = r / K); GroupNorm becomes
 *     dy = gamma rstd (dx - mean_g(dx) - xh mean_g(dx xh)),  xh = (x - mean) rstd from the tape's x and (mean, rstd),
 * GELU becomes da = du gelu'(u) with the derivative as the backward writes it, the channel scale dxm = dx1 (1 + m).
 * Order of the sums: the GroupNorm JVP is one 256-thread block per (group, row); dx xh is a rounded fp32 product (never
 * contracted into the sum); a thread adds its elements i = tid, tid + 256, ... ascending in fp32, the wave is summed by
 * the fixed cross-lane sequence of the training kernels (t_wave_sum), the four waves as (w0 + w1) + (w2 + w3); where a
 * group holds one value, dx - mean_g(dx) is exactly 0.  No atomics; scalar accesses; bit-reproducible.  [t0, t0 + n) in
 * one call has the bits of [t0, t0 + s) then [t0 + s, t0 + n).  The tiling of the convolutions follows B*K, so one
 * (sample, tangent) run alone agrees with its row of a batch to rounding, not bit for bit.
 * Workspace (lns_train_tangent_workspace_bytes(e, B, h, w, T, K); needs no GPU): lns_train_workspace_bytes' layout under
 * the engine's current "train_wgrad", no offset moved | four tangent tensors of 4 * B * K * D * h * w bytes | one latent
 * tangent of 4 * B * K * c * h * w bytes -- each part rounded up to 256 bytes.  The forward must be given this workspace.
 * Refusals, decided on the host in this order before anything is enqueued: null e / params / v (size query: bytes); K
 * outside 1 .. LNS_TANGENT_MAX; B < 1 or B*K beyond the batch limit; t0 < 0, nsteps < 1 or t0 + nsteps > T; no propagator
 * (LNS_ESTATE); v / jv_out / workspace not device memory of one device; workspace null or short (LNS_ENOMEM naming the
 * bytes); a null propagator parameter pointer.  No host synchronisation, allocation or host copy inside the call. */
#define LNS_TANGENT_MAX 32
int lns_train_tangent_workspace_bytes(lns_engine* e, int B, int h, int w, int T, int K, size_t* bytes);
int lns_train_tangent(lns_engine* e, const float* const* params, int B, int h, int w, int T, int K, int t0, int nsteps,
                      float* v, float* jv_out_or_null, void* workspace, size_t workspace_bytes, void* stream);

/* One pass of modified Gram-Schmidt over the K vectors of every sample, v [B,K,n] fp32 in place: for k ascending, for
 * j < k ascending
 *     r_jk = <q_j, v_k>,   v_k[i] = (float)((double)v_k[i] - r_jk * (double)q_j[i])        (rounded once per projection;
 * the v_k of an inner product is the one the earlier projections left), then
 *     R_kk = sqrt(<v_k, v_k>),   q_k[i] = (float)((double)v_k[i] / R_kk)                   (rounded once).
 * Order: every product and sum in double (a product of two floats is exact there), as lns_loss_obs_mse sums: one
 * 256-thread block per sample, a thread adds i = tid, tid + 256, ... ascending, the wave is a butterfly with neighbours
 * first, the four waves (w0 + w1) + (w2 + w3).  r [B,K,K] double (nullable): the upper triangle, zeros below;
 * logr_acc [B,K] double (nullable): += log(R_kk) -- the caller zeroes it.  R_kk == 0: q_k = 0 and the contribution is
 * -inf; no NaN.  Scalar accesses: the bits do not depend on the pointer's alignment.  Refuses K outside
 * 1 .. LNS_TANGENT_MAX, n < 1, B < 1 (message: lns_create_error()); never synchronises. */
int lns_op_orthonormalize(float* v, int B, int K, int64_t n, double* r_or_null, double* logr_acc_or_null, void* stream);

/* ---- diagnostics -------------------------------------------------------- */
/* Layer trace: when enabled the run calls synchronise after every reference
 * module boundary and keep a host copy of its output (tests compare them with
 * the oracle layer by layer).  Slow; never enable in production. */
int lns_trace_enable(lns_engine* e, int on);
int lns_trace_count(const lns_engine* e);
int lns_trace_info(const lns_engine* e, int index, char* name, int name_capacity,
                   int64_t* shape /* [4] */);
int lns_trace_copy(const lns_engine* e, int index, float* host_out);

/* Kernel-level timing: after a run call with timing enabled, per-kernel-class
 * elapsed milliseconds measured with HIP events on the call's stream. */
int lns_timing_enable(lns_engine* e, int on);
int lns_timing_count(const lns_engine* e);
int lns_timing_info(const lns_engine* e, int index, char* name, int name_capacity,
                    double* total_ms, int64_t* launches, double* flops, double* bytes);
/* Records named "class/form" follow the per-class ones: the same launches split by kernel form (nine-tap / four-tap /
 * fp32-MFMA 3x3, streaming / input-stationary / fused 1x1, ...).  mfma_flops: FLOP the record's launches EXECUTED on the
 * matrix pipe -- the three products of the split-operand scheme and every padded tap slot, channel and tile included --
 * in FLOP of the form's instruction ("f16x2 ...": fp16 MFMA, "fp32 MFMA ...": fp32 MFMA); `flops` above stays algorithmic. */
int lns_timing_mfma_flops(const lns_engine* e, int index, double* mfma_flops);
/* (index -1: instead of a record's FLOP, the per-launch overhead in MICROSECONDS that the engine measured for its
 *  (event, launch, event) timing around empty launches and subtracted from every timed launch; -1000 before the first timed run) */

/* Build-time features of this library: "experimental" = compiled with -DLNS_EXPERIMENTAL (the measured-slower kernel
 * forms behind op-level variants 15 / 16 / 18 / 19 exist; the shipped library does not carry them); "train_wgrad_split" = the
 * batch-parallel weight gradient (option "train_wgrad", lns_op_conv_wgrad) is there; "train_clip" = lns_train_step_clip and
 * the gradient-norm / update calls are there; "train_ops" = lns_op_groupnorm_train, lns_op_gelu_grad and lns_op_bias_grad
 * are there; "rollout_select" = lns_rollout_select & co. are there; "rollout_ensemble" = lns_rollout_latent_ensemble,
 * its size query and lns_op_ensemble_stats are there; "ensemble_score" = lns_rollout_latent_ensemble_eval and
 * lns_op_ensemble_score are there; "eval_spectrum" = lns_rollout_eval_spectrum, lns_rollout_latent_eval_spectrum,
 * lns_op_energy_spectrum and lns_spectrum_bins are there; "spectrum_basis" = lns_spectrum_bins_basis,
 * lns_op_energy_spectrum_basis and the option "spectrum_basis" are there; "eval_stats" = lns_rollout_eval_stats,
 * lns_rollout_latent_eval_stats and lns_op_field_stats are there; "eval_maps" = lns_rollout_eval_maps,
 * lns_rollout_latent_eval_maps, their size query, lns_op_time_maps and lns_time_maps_state_bytes are there;
 * "op_conv_gn" = lns_op_conv_gn is there; "op_fa_fused" = lns_op_fa_fused is there; "eval_attrib" = lns_rollout_eval_attrib, lns_rollout_latent_eval_attrib, their
 * size query, lns_autoencode_eval, its size query, lns_op_eval_attrib and lns_op_latent_err are there;
 * "ensemble_quantiles" = lns_rollout_latent_ensemble_quantiles and lns_op_ensemble_quantiles are there;
 * "ensemble_exceed" = lns_rollout_latent_ensemble_exceed and lns_op_ensemble_exceed are there; "op_fa_axis" =
 * lns_op_fa_reducer, lns_op_fa_lrk, lns_op_ln_pe, lns_op_apply, lns_rotary_table and the two fit predicates are there;
 * "eval_flow" = lns_rollout_eval_flow, lns_rollout_latent_eval_flow, lns_op_flow_stats and lns_op_vorticity are there;
 * "latent_fit" = lns_train_backward_ex, lns_loss_obs_mse, its size query, lns_fit_step and its size query are there;
 * "rollout_tangent" = lns_train_tangent, its size query and lns_op_orthonormalize are there; "fit_gauss_newton" =
 * lns_train_gn_product, lns_fit_gn_step, their size queries, lns_op_cg_start and lns_op_cg_update are there; "ensemble_etkf" =
 * lns_rollout_latent_ensemble_analysis, its size query, lns_op_ensemble_obs_gram, lns_op_etkf_transform and
 * lns_op_ensemble_transform are there; "ensemble_letkf" = lns_rollout_latent_ensemble_analysis_local, its size query,
 * lns_op_ensemble_patch_gram, lns_op_letkf_combine and lns_op_ensemble_transform_local are there.
 * 1 / 0; -1: unknown name.
 * (No reference counterpart: the reference is pure Python.) */
int lns_build_has(const char* feature);

/* ---- kernel-level entry points (unit tests of the HIP kernels) ---------- */
/* General fused convolution (the implicit-GEMM MFMA kernel):
 *   y = act_out( conv(act_in(x * scale + shift)) + bias + badd ) + residual
 * x [B,Cin,Hin,Win] optionally nearest-resized to (Hv,Wv) before padding;
 * w [Cout,Cin,k,k] HOST pointer; ss [B,Cin,2] device (scale,shift) or NULL;
 * act: 0 none, 1 swish, 2 gelu.  tile_variant <0 = automatic; >= 0: a kernel / tile form (lns_kernels.h ConvVariant) in
 * the low byte, plus tensor layouts: | 0x100 = x is channel-octet-interleaved ("OCT8": [Cin/8][Hin*Win][8] per sample,
 * Cin % 8 == 0), | 0x200 = y and residual are OCT8 ([Cout/8][Hout*Wout][8]) -- the engine's layout of conv <-> conv
 * intermediates.
 * amax_out (device, [B][16] unsigned, zero-initialised by the caller, or NULL): the maximum over the 16 words of
 * sample b is the IEEE bit pattern of max |y[b]| -- the side channel from which the split-operand (f16x2) kernels of a plan derive their per-sample
 * power-of-two activation scale.  The entry point computes the same quantity for x itself before the launch. */
int lns_op_conv2d(const float* x, int B, int Cin, int Hin, int Win, int Hv, int Wv,
                  const float* w_host, const float* bias_host, int Cout, int ksize, int stride,
                  int dilation, int pad_t, int pad_b, int pad_l, int pad_r, int mode_y, int mode_x,
                  const float* ss, int act_in, int act_out, const float* residual,
                  const float* badd, float* y, int tile_variant, void* stream, unsigned* amax_out);
/* GroupNorm from the tile statistics of the convolution that produced its input (unit tests of that path; "op_conv_gn" in
 * lns_build_has): a producer convolution leaves per-(sample, 128-pixel tile, channel) (mean, M2) partials in its epilogue,
 * and they are merged (a) by the finalize kernels into a [B,Cout,2] (scale, shift) table and / or (b) in the prologue of a
 * consumer convolution, which needs no launch of its own ("the fold").  Whether a producer carries the statistics, over
 * which pixel counts (exact 128-pixel tiles / one ragged tile / ragged tiles of a larger plane) and whether the fold is
 * allowed is the planner's own rule, called by this entry point and the planner alike; a combination a plan never holds
 * is LNS_EINVAL (message: lns_create_error()).  Existing launchers only.  Every check precedes the first launch; the call
 * synchronises `stream`.
 *   producer   lns_op_conv2d's arguments (x .. tile_variant, OCT8 bits included), y its stored output
 *   part_out   device [B][tiles][Cout][2] or NULL: a copy of the producer's partials
 *   part_in    device, same layout, or NULL: merged INSTEAD of the producer's (crafted (mean, M2) sets)
 *   geom       host int[8] or NULL: tiles_x, tiles_y, log2 of the tile width, flat (1: a tile is 128 consecutive pixels of
 *              the flattened plane, 1x1 producers), phase multiplier (4: upsampling form, partial (ty * tiles_x + tx) * 4 +
 *              2 * py + px covers output pixels (2 sy + py, 2 sx + px) of source tile (ty, tx); else 1), mode (0 exact,
 *              1 one ragged tile, 2 ragged tiles), foldable (0 / 1), tiles (= tiles_x * tiles_y * phase multiplier)
 *   GroupNorm  groups, eps, gamma / beta HOST [Cout], premul device [B][Cout] or NULL (statistics of y * premul)
 *   ss_out     device [B][Cout][2] or NULL: merge form (a)
 *   consumer   merge form (b), when w2_host != NULL: y2 = conv2(act_in2(GroupNorm(y))) + bias2, a stride-1 "same"
 *              convolution [Cout2,Cout,ksize2,ksize2] with the producer's padding modes, its GroupNorm
 *              arguments set as the planner sets them; variant2 11 / 13 (3x3) or 7 (streaming 1x1), | 0x100 exactly when
 *              the producer stores OCT8 (3x3 consumers only: the 1x1 kernel reads planar tensors); act_in2 0 / 1.  Refused
 *              where the rule says the merge cannot be folded. */
typedef struct lns_conv_gn_args {
    const float* x; int B, Cin, Hin, Win, Hv, Wv;
    const float* w_host; const float* bias_host; int Cout, ksize, stride, dilation, pad_t, pad_b, pad_l, pad_r, mode_y, mode_x;
    const float* ss; int act_in, act_out; const float* residual; const float* badd; float* y; int tile_variant;
    float* part_out; const float* part_in; int* geom;
    int groups; float eps; const float* gamma_host; const float* beta_host; const float* premul;
    float* ss_out;
    const float* w2_host; const float* bias2_host; int Cout2, ksize2, act_in2, variant2; float* y2;
} lns_conv_gn_args;
int lns_op_conv_gn(const lns_conv_gn_args* args, void* stream);
/* FABlock2D with in_proj inside the sandwich (unit tests of csrc/fa_fused.inc; "op_fa_fused" in lns_build_has): the input
 * split pre-pass and the fused kernel on their own, their arguments set as the planner sets them,
 *   G = x * scale + shift,  P[h * dim_head + d] = sum_c W[h * dim_head + d][c] G[c],  Y = Kx[b][h] P Ky[b][h]^T,
 *   out = (Y - mean) / sqrt(var_biased + eps) per plane when instnorm, else Y.
 * Existing launchers only: the call allocates the split input and the max |G| words, packs W with the planner's scales,
 * runs the two launches, synchronises `stream` and frees what it allocated.  Every check precedes the first HIP call
 * (LNS_EINVAL, message lns_create_error() starting "fa_fused: "): null x / w_host / kx / ky / out, B or heads outside 1..65535, a shape
 * without a fused kernel (64 x 64 planes with 64 channels, 32 x 32 with 64 or 128; dim_head a multiple of 16), a gpb that
 * does not divide dim_head / 16, form outside 0..2 or nonzero at 32 x 32, a bound that is not > 0, x_bs < Cin * H * W.
 *   x          device, B samples of [Cin][H][W], x_bs floats apart
 *   ss         device [B][Cin][2] (scale, shift), or NULL: identity
 *   bound      a bound of |G| (inside a plan: max |gamma| sqrt(Cin H W) + max |beta| of the in_norm GroupNorm): G is split at
 *              the power of two that puts it at 2^14 .. 2^15
 *   w_host     HOST [heads * dim_head][Cin]
 *   kx, ky     device [B][heads][H][H], [B][heads][W][W]
 *   form       64 x 64: 0 the double-buffered kernel (shipped), 1 the single-buffered one, 2 the generic one; 32 x 32: 0
 *   gpb        plane groups (of 16) a block walks; 0 = the planner's automatic choice.  b_rev: blocks take samples last to first
 *   out        device [B][heads * dim_head][H][W]
 *   amax_out   device [B] float or NULL: max |G| of each sample as the pre-pass recorded it (the maximum over its 16 words) */
typedef struct lns_fa_fused_args {
    const float* x; int64_t x_bs; const float* ss; float bound;
    const float* w_host; const float* kx; const float* ky;
    int B, heads, dim_head, Cin, H, W; float eps; int instnorm, form, gpb, b_rev;
    float* out; float* amax_out;
} lns_fa_fused_args;
int lns_op_fa_fused(const lns_fa_fused_args* args, void* stream);
/* The kernels that build a FABlock's Kx / Ky, the SABlock pre-norm and the GroupNorm materialisation at op level (unit tests;
 * "op_fa_axis" in lns_build_has).  Existing launchers only, their arguments set as the planner sets them.  Device pointers
 * are fp32; weights are HOST pointers in the reference's state_dict layout ([out][in]), transposed by the planner's own
 * helper.  Every check precedes the first HIP call (LNS_EINVAL, message lns_create_error() starting "fa_reducer: ",
 * "fa_lrk: ", "ln_pe: ", "apply: "); each call synchronises `stream` and frees what it allocated.
 *
 * Supported shapes, the planner's own predicates (a plan whose FABlock has none fails at plan time, naming the layer):
 *   lns_fa_reducer_fits(C, Hid, Out, merged)   the MFMA form (C, Hid multiples of 32, C <= 256, LDS (max(C Hid, 128 Hid, 128 Out)
 *                                              + 33 (2 C + Hid) + 256) * 4 <= 160 KB) or, one axis per launch only, the
 *                                              scalar form (LDS (C C + C Hid + Hid Out + 16 (2 C + Hid)) * 4 <= 160 KB)
 *   lns_fa_lrk_fits(DK, n)                     DK even, LDS 2 DK (n rounded up to 32) * 4 <= 160 KB
 * 1 / 0; no device needed.
 *
 * lns_op_fa_reducer: PoolingReducer on pooled rows, u = W2 gelu(W1 LayerNorm(W_in m)) + b2 (LayerNorm over C, eps 1e-5).
 *   mx, my       device [B][nx][C], [B][ny][C]; my NULL: the x axis alone (every *_y member is ignored)
 *   to_in_*      HOST [C][C];  ln_g_*, ln_b_* HOST [C];  w1_* HOST [Hid][C];  w2_* HOST [Out][Hid];  b2_* HOST [Out]
 *   ux, uy       device [B][Out][nx], [B][Out][ny]
 *   amax_x/_y    device [B] float or NULL: max |u| of each sample as the kernel recorded it (the maximum over its 16 words)
 *   form         0: both axes in one launch (needs both; MFMA form only), 1: one launch per axis (MFMA form where it fits,
 *                else the scalar form).  Hid is a parameter; the planner passes 2 C. */
typedef struct lns_fa_reducer_args {
    const float* mx; const float* my; int B, nx, ny, C, Hid, Out, form;
    const float* to_in_x; const float* ln_g_x; const float* ln_b_x; const float* w1_x; const float* w2_x; const float* b2_x;
    const float* to_in_y; const float* ln_g_y; const float* ln_b_y; const float* w1_y; const float* w2_y; const float* b2_y;
    float* ux; float* uy; float* amax_x; float* amax_y;
} lns_fa_reducer_args;
int lns_fa_reducer_fits(int C, int Hid, int Out, int merged);
int lns_op_fa_reducer(const lns_fa_reducer_args* args, void* stream);
/* lns_op_fa_lrk: LowRankKernel after to_qk, K[b][h] = rot(q[b][h]) rot(k[b][h])^T, no softmax, no scaling.
 *   qk_x, qk_y   device [B][2 heads DK][n]: q of head h in channels h DK .., k in (heads + h) DK ..; qk_y NULL: the x axis alone
 *   inv_freq_*   HOST [DK / 2]: the rotary frequencies; the table is lns_rotary_table's
 *   kx, ky       device [B][heads][n][n]
 *   form         0: both axes in one launch (needs both, with the same B, heads and DK), 1: one launch per axis */
typedef struct lns_fa_lrk_args {
    const float* qk_x; const float* qk_y; int B_x, heads_x, DK_x, nx, B_y, heads_y, DK_y, ny, form;
    const float* inv_freq_x; const float* inv_freq_y; float* kx; float* ky;
} lns_fa_lrk_args;
int lns_fa_lrk_fits(int DK, int n);
int lns_op_fa_lrk(const lns_fa_lrk_args* args, void* stream);
/* The rotary table of a plan, no device needed: pos = torch.linspace(0, 1, n) in its float32 arithmetic, f = (pos * 64) *
 * inv_freq[d] in float32, out_host [half][n][2] = (float)cos((double)f), (float)sin((double)f). */
int lns_rotary_table(int n, const float* inv_freq_host, int half, float* out_host);
/* SABlock pre-norm: h[b][c][i] = LayerNorm_c(x[b][:][i]) gamma[c] + beta[c] + pe[i][c].  x device, sample b at x + b * x_bs
 * floats, [C][n]; gamma, beta HOST [C]; pe_host HOST [pe_len][C] (pe_len >= n) or NULL; h device [B][C][n].
 * bound_out (HOST float, nullable): the bound of |h| the planner hands the consumer of h,
 * sqrt(C) max|gamma| + max|beta| + max|pe|. */
int lns_op_ln_pe(const float* x, int64_t x_bs, int B, int C, int n, const float* gamma_host, const float* beta_host,
                 const float* pe_host, int pe_len, float eps, float* h, float* bound_out, void* stream);
/* y[b][c] = act(x[b][c] * scale + shift): x device, sample b at x + b * x_bs floats, [C][HW]; ss device [B][C][2] or NULL:
 * identity; act 0 none, 1 swish, 2 gelu, 3 relu, 4 tanh, 5 sigmoid; y device [B][C][HW]; amax_out device [B][16] unsigned,
 * zero-initialised by the caller, or NULL (lns_op_conv2d's side channel: the maximum over the 16 words is max |y[b]|). */
int lns_op_apply(const float* x, int64_t x_bs, const float* ss, int act, int B, int C, int HW, float* y, unsigned* amax_out,
                 void* stream);
/* Diagnostic: runs two convolutions (GroupNorm+Swish prologue, circular padding, stride 1) repeatedly on two HIP
 * streams so that their workgroups share compute units, and counts output words that differ from what each
 * convolution produces alone.  variant_*: tile variant as in lns_op_conv2d (-1 automatic, 6 = bf16x3 3x3 kernel). */
int lns_op_conv_pair_stress(int B, int H, int W, int cin_a, int cout_a, int ksize_a, int variant_a, int cin_b, int cout_b,
                            int ksize_b, int variant_b, int rounds, int launches, long long* mismatches_a,
                            long long* mismatches_b);

/* Weight gradient of a stride-1 "same" convolution (ksize 1 or 3, dilation d, padding d * (ksize - 1) / 2 per side):
 *   dw[co][ci][ty][tx] (+)= sum_b sum_{y,x} dy[b][co][y][x] * xpad[b][ci][y + ty*d][x + tx*d]
 * dy [B,Cout,H,W], x [B,Cin,H,W], dw [Cout,Cin,ksize,ksize]: device fp32; pad_y / pad_x: LNS_PAD_ZEROS / LNS_PAD_CIRCULAR per
 * axis; accumulate 1: added to the value already in dw.  form 0: one block per output tile; form 1: batch-parallel (the
 * two kernels of option "train_wgrad"), which needs `scratch` (device) of lns_op_conv_wgrad_scratch_bytes(...) bytes =
 * S * Cout * Cin * ksize^2 floats rounded up to 64 floats, S a function of (B, Cin, Cout, H, W, ksize) only; form 0: 0 bytes,
 * scratch may be NULL.  Exact-fp32 matrix instruction in both forms.  Every argument check precedes the first launch
 * (LNS_EINVAL; LNS_ENOMEM for a short scratch; message: lns_create_error()); the call synchronises `stream`.
 * lns_op_conv_wgrad_scratch_bytes needs no device. */
int lns_op_conv_wgrad_scratch_bytes(int B, int Cin, int Cout, int H, int W, int ksize, int form, size_t* bytes);
int lns_op_conv_wgrad(const float* dy, const float* x, int B, int Cin, int Cout, int H, int W, int ksize, int dilation,
                      int pad_y, int pad_x, int form, int accumulate, float* dw, void* scratch, size_t scratch_bytes,
                      void* stream);

/* The elementwise and reduction kernels of the training rollout's backward pass on their own (unit tests of their input
 * domain): the launchers lns_train_forward / lns_train_backward use, nothing added.  All pointers DEVICE fp32; argument
 * checks precede the first launch (LNS_EINVAL; message: lns_create_error()); each call synchronises `stream`.
 *
 * Training-form GroupNorm (nn.GroupNorm, biased variance, two-pass statistics).  Forward, always:
 *   y [B,C,HW] = (x - mean) rstd gamma + beta,  stats [B,groups,2] = (mean, rstd) per (sample, group).
 * Backward, when dy [B,C,HW] is given, from the stats just written:
 *   dx [B,C,HW] = (add ? add : 0) + rstd (gamma dy - mean_g(gamma dy) - xhat mean_g(gamma dy xhat))
 *   dgamma[c] (+)= sum_b sum_p dy xhat,  dbeta[c] (+)= sum_b sum_p dy      (accumulate 1: added to what dgamma / dbeta hold)
 * through the per-sample partials `part` [B,C,2] (scratch) and their reduction over the batch in ascending order.
 * add: the gradient arriving over a skip connection, or NULL.  dy NULL: forward only (dx .. part are not read). */
int lns_op_groupnorm_train(const float* x, int B, int C, int HW, int groups, float eps, const float* gamma, const float* beta,
                           float* y, float* stats, const float* dy, const float* add, float* dx, float* dgamma, float* dbeta,
                           int accumulate, float* part, void* stream);
/* du[i] = dy[i] * d/du GELU(u[i]), exact-erf GELU (nn.GELU default): Phi(u) + u phi(u).  1 <= n <= 2^40. */
int lns_op_gelu_grad(const float* dy, const float* u, float* du, int64_t n, void* stream);
/* db[c] (+)= sum_b sum_p dy[b][c][p], dy [B,C,HW]; one fixed summation order: bit-reproducible. */
int lns_op_bias_grad(const float* dy, int B, int C, int HW, float* db, int accumulate, void* stream);

/* The reduction kernel of lns_rollout_latent_ensemble on its own: frames [B][M][per] -> mean [B][per] and var [B][per]
 * (nullable; var != NULL with M < 2 is LNS_EINVAL) by the statement written there.  16-byte accesses when the three
 * pointers are 16-byte aligned and per is a multiple of 4, one element at a time otherwise: the bits do not depend on it.
 * B in 1..65535, M in 1..65536, per in 1..2^40.  Checks precede the launch (message: lns_create_error()); the call
 * synchronises `stream`. */
int lns_op_ensemble_stats(const float* frames, int B, int M, int64_t per, float* mean, float* var /* nullable */, void* stream);

/* The two kernels of lns_rollout_latent_ensemble_eval on stored member fields, without an engine: frames
 * [n][B][M][C][H][W] (the layout of a frame buffer), y [B][n][C][H][W] -> scores_out [B][n][C][4], seq_out (nullable)
 * [B][C][4], rank_out (nullable) [B][n][C][M+1] by the statement written there.  pixel_out (nullable, for tests)
 * [n][B][C][H*W][4]: mu, var, crps and (float)rank of every pixel.  2 <= M <= 128, B in 1..65535, n * B * C < 2^31; the
 * per-channel form needs C <= 8.  Checks precede the launch (message: lns_create_error()); the call synchronises `stream`. */
int lns_op_ensemble_score(const float* frames, const float* y, int n, int B, int M, int C, int H, int W,
                          const lns_eval_spec* spec, float* scores_out, float* seq_out, int32_t* rank_out,
                          float* pixel_out, void* stream);

/* The kernel of lns_rollout_latent_ensemble_quantiles on stored member fields, without an engine: frames
 * [n][B][M][C][H][W] (the layout of a frame buffer) -> quant_out [B][n][n_q][C][H][W] and prob_out [B][n][n_thr][C][H][W] by the
 * statement written there; norm nullable (the members as they are).  1 <= M <= 128, B in 1..65535, n * B * C < 2^31; the
 * per-channel form needs C <= 8.  Checks precede the launch (message: lns_create_error()); the call synchronises `stream`. */
int lns_op_ensemble_quantiles(const float* frames, int n, int B, int M, int C, int H, int W,
                              const lns_ensemble_quantile_spec* qspec, const lns_eval_spec* norm /* nullable */,
                              float* quant_out, float* prob_out, void* stream);

/* The kernel of lns_rollout_latent_ensemble_exceed on stored member fields, without an engine: frames [n][B][M][C][H][W]
 * (the layout of a frame buffer) against y [B][n][C][H][W] -> table_out [B][n][n_thr][C][2][M+1] (int32) by the statement
 * written there; norm nullable (members and truth as they are).  The call zeroes the table ahead of its launch: the whole
 * table is overwritten.  1 <= M <= 128, B in 1..65535, C <= 8, H * W <= 2^30, n * B * C < 2^31.  Checks precede the launch
 * (message: lns_create_error()); the call synchronises `stream`. */
int lns_op_ensemble_exceed(const float* frames, const float* y, int n, int B, int M, int C, int H, int W,
                           const lns_ensemble_exceed_spec* xspec, const lns_eval_spec* norm /* nullable */,
                           int32_t* table_out, void* stream);

/* The three kernels of lns_rollout_latent_ensemble_analysis without an engine, by the statement written there.
 * lns_op_ensemble_obs_gram: frames [n][B][M][C][H][W] (the layout of a frame buffer), y_obs [B][n][C][H][W], rinv with its two
 * strides, norm nullable -> S_out [B][n][M][M] (full, symmetric), g_out [B][n][M], stat_out [B][n][3], all double; the slice
 * partials live in device memory the call owns, and the call synchronises `stream`.  Refusals in this order: frames, y_obs or
 * rinv null; an output null; norm of the wrong size; M outside 2 .. 64; the shape (as lns_op_ensemble_exceed); a negative
 * stride; the per-channel norm with C > 8.
 * lns_op_etkf_transform: S [B][n][M][M], g [B][n][M] -> X [B][M][M], wbar [B][M], lam [B][M] (double), status [B] (int32); one
 * block per sample, no host read, never synchronises.  Refusals: S or g null; an output null; M outside 2 .. 64; B, n < 1;
 * rho < 1 or not finite.
 * lns_op_ensemble_transform: z [B][M][n] fp32, X [B][M][M] double -> out [B][M][n], which may be z; never synchronises.
 * Refusals: a null pointer; M outside 2 .. 64; B outside 1..65535 or n outside 1..2^38.
 * Messages: lns_create_error(). */
int lns_op_ensemble_obs_gram(const float* frames, const float* y_obs, const float* rinv, int64_t rinv_bs, int64_t rinv_ss,
                             int n, int B, int M, int C, int H, int W, const lns_eval_spec* norm /* nullable */,
                             double* S_out, double* g_out, double* stat_out, void* stream);
int lns_op_etkf_transform(const double* S, const double* g, int B, int n, int M, double rho, double* X, double* wbar,
                          double* lam, int32_t* status, void* stream);
int lns_op_ensemble_transform(const float* z, const double* X, int B, int M, int64_t n, float* out, void* stream);

/* The three kernels that lns_rollout_latent_ensemble_analysis_local adds, without an engine, by the statement written there
 * (the transform between them is lns_op_etkf_transform on S_local viewed as [B * h * w][1][M][M]).  None synchronises.
 * lns_op_ensemble_patch_gram: frames, y_obs, rinv, norm as lns_op_ensemble_obs_gram, the [C][H][W] frame cut into h x w patches
 * -> part_out [B][n][h*w][M*M + M + 3] double: per patch G [M][M] (full, symmetric), g [M], stat [3]; an empty patch: zeros.
 * Refusals in this order: frames, y_obs or rinv null; part_out null; norm of the wrong size; M outside 2 .. 64; the shape (as
 * lns_op_ensemble_exceed); n > 65535; h or w < 1 or h * w > 4096; a negative stride; the per-channel norm with C > 8.
 * lns_op_letkf_combine: part [B][n][h*w][M*M + M + 3] -> S_local [B][h*w][M][M], g_local [B][h*w][M], S_glob [B][M][M], g_glob
 * [B][M], stat [B][n][3] (nullable).  Refusals: part null; an output but stat null; M outside 2 .. 64; B outside 1..65535 or
 * n < 1; the grid; loc_radius not finite or <= 0; bc_y / bc_x not LNS_FLOW_PERIODIC / LNS_FLOW_WALL.
 * lns_op_ensemble_transform_local: z [B][M][c][h][w] fp32, X_local [B][h*w][M][M] double -> out [B][M][c][h][w], which may be z.
 * Refusals: a null pointer; M outside 2 .. 64; B outside 1..65535 or c outside 1..65536; the grid.
 * Messages: lns_create_error(). */
int lns_op_ensemble_patch_gram(const float* frames, const float* y_obs, const float* rinv, int64_t rinv_bs, int64_t rinv_ss,
                               int n, int B, int M, int C, int H, int W, int h, int w, const lns_eval_spec* norm /* nullable */,
                               double* part_out, void* stream);
int lns_op_letkf_combine(const double* part, int B, int n, int M, int h, int w, double loc_radius, int bc_y, int bc_x,
                         double* S_local, double* g_local, double* S_glob, double* g_glob, double* stat /* nullable */,
                         void* stream);
int lns_op_ensemble_transform_local(const float* z, const double* X_local, int B, int M, int c, int h, int w, float* out,
                                    void* stream);

/* The spectrum kernel of lns_rollout_eval_spectrum on stored fields, without an engine: yhat and y (nullable) [B][T][C][H][W],
 * normalised -> out [B][T][C][K][S], K = 3 (forecast, truth, error) when y is given, K = 1 (the forecast's row, same bits) when
 * it is NULL; S = lns_spectrum_bins(H, W).  The per-plane body is the streaming call's (one device function).  B * T * C < 2^31;
 * the per-channel form needs C <= 8.  Checks precede the launch (message: lns_create_error()); the call synchronises `stream`. */
int lns_op_energy_spectrum(const float* yhat, const float* y /* nullable */, int B, int T, int C, int H, int W,
                           const lns_eval_spec* spec, float* out, void* stream);
/* The same with a basis per axis (LNS_SPECTRUM_DFT / LNS_SPECTRUM_DCT; anything else: LNS_EINVAL ahead of the launch):
 * S = lns_spectrum_bins_basis(H, W, basis_y, basis_x).  (.., 0, 0) is lns_op_energy_spectrum, bit for bit. */
int lns_op_energy_spectrum_basis(const float* yhat, const float* y /* nullable */, int B, int T, int C, int H, int W,
                                 const lns_eval_spec* spec, float* out, void* stream, int basis_y, int basis_x);

/* The statistics kernel of lns_rollout_eval_stats on stored fields, without an engine: yhat and y [B][T][C][H][W],
 * normalised -> stats_out [B][T][C][12] and, with hspec and hist_out, hist_out [B][T][C][2][nbins + 2].  The per-plane body
 * is the streaming call's (one device function).  H * W <= 2^30, B * T * C < 2^31; the per-channel form and histograms need
 * C <= 8.  Checks precede the launch (message: lns_create_error()); the call synchronises `stream`. */
int lns_op_field_stats(const float* yhat, const float* y, int B, int T, int C, int H, int W, const lns_eval_spec* spec,
                       const lns_stats_spec* hspec /* nullable */, float* stats_out, int32_t* hist_out /* nullable */,
                       void* stream);

/* The flow kernels of lns_rollout_eval_flow on stored fields, without an engine.  lns_op_flow_stats: yhat and y
 * [B][T][C][H][W], normalised -> flow_out [B][T][12] and, with fspec->nbins > 0 and hist_out, hist_out [B][T][2][nbins + 2].
 * lns_op_vorticity: fields [B][T][C][H][W], normalised -> vort_out [B][T][H][W], the vorticity of every frame (of a forecast
 * or of the truth).  The per-frame bodies are the streaming call's (one device function).  C >= 2, H * W <= 2^30,
 * B * T < 2^24; the per-channel form needs C <= 8.  Checks precede the launch (message: lns_create_error()): the pointers,
 * spec, the shape, then fspec in the order written for lns_rollout_eval_flow; the calls synchronise `stream`. */
int lns_op_flow_stats(const float* yhat, const float* y, int B, int T, int C, int H, int W, const lns_eval_spec* spec,
                      const lns_flow_spec* fspec, float* flow_out, int32_t* hist_out /* nullable */, void* stream);
int lns_op_vorticity(const float* fields, int B, int T, int C, int H, int W, const lns_eval_spec* spec,
                     const lns_flow_spec* fspec, float* vort_out, void* stream);

/* The time maps of lns_rollout_eval_maps on stored fields, without an engine: yhat and y [B][T][C][H][W], normalised ->
 * maps_out [B][C][7][H][W] over the steps map_from, map_from + map_every, ... below T (the horizon is T, K is y[b][0]).
 * `state` is device memory of at least lns_time_maps_state_bytes(B, C, H, W) = 52 B C H W rounded up to 256 bytes, 8-byte
 * aligned; the call clears it, accumulates (the streaming call's device function) and finishes.  H * W <= 2^30, B <= 65535;
 * the per-channel form needs C <= 8.  Checks precede the launches (message: lns_create_error()): LNS_EINVAL, or LNS_ENOMEM
 * for a state_bytes below the need; the call synchronises `stream`. */
int lns_time_maps_state_bytes(int B, int C, int H, int W, size_t* bytes);
int lns_op_time_maps(const float* yhat, const float* y, int B, int T, int C, int H, int W, const lns_eval_spec* spec,
                     int map_from, int map_every, float* maps_out, void* state, size_t state_bytes, void* stream);

/* The attribution kernels of lns_rollout_eval_attrib on stored fields, without an engine: yhat (forecast), r (reconstruction
 * of the truth) and y [B][T][C][H][W], normalised -> prop_frame / cross_frame [B][T][C], prop_seq / cross_seq [B][C] (each
 * nullable, at least one set).  The per-plane body and the finish kernel are the streaming call's.
 * Scratch: the partial sums (3 B T C floats) are allocated by the call with hipMalloc and freed before it returns.  H * W <= 2^30, B * T * C < 2^31; the per-channel form
 * needs C <= 8.  Checks precede the launches (message: lns_create_error()); the call synchronises `stream`. */
int lns_op_eval_attrib(const float* yhat, const float* r, const float* y, int B, int T, int C, int H, int W,
                       const lns_eval_spec* spec, float* prop_frame, float* prop_seq, float* cross_frame, float* cross_seq,
                       void* stream);

/* The latent-drift kernel of lns_rollout_eval_attrib on one stored group, without an engine: z [T][B][zper] (a ring group's
 * layout, any alignment) against ztrue [T][B][zstride] (zstride a multiple of 4 floats >= zper, ztrue 16-byte aligned) ->
 * frame_out [B][T], seq_out [B] (either nullable): the bits of lns_metric_rel_l2 on the latents stored as [B][T][1][1][zper]
 * with mean 0, std 1.  Scratch (2 B T floats) is allocated and freed by the call; it synchronises `stream`. */
int lns_op_latent_err(const float* z, const float* ztrue, int B, int T, int zper, int64_t zstride, float eps, float* frame_out,
                      float* seq_out, void* stream);

/* GroupNorm statistics -> per-(b,c) (scale,shift) such that norm(x) = x*scale+shift. */
int lns_op_groupnorm_stats(const float* x, int B, int C, int HW, int groups, float eps,
                           const float* gamma_host, const float* beta_host, const float* premul,
                           float* ss, void* stream);
/* softmax attention: qkv [B,3*heads*dim_head,n] channel-major -> o [B,heads*dim_head,n] */
int lns_op_attention(const float* qkv, int B, int heads, int dim_head, int n, float scale,
                     float* o, void* stream);
/* FABlock2D core: for every channel plane P of u [B,heads*C,H,W]:
 *   P <- instance_norm( Kx[b,h] . P . Ky[b,h]^T ), kx [B,heads,H,H], ky [B,heads,W,W] */
int lns_op_fa_sandwich(const float* u, const float* kx, const float* ky, int B, int heads, int C,
                       int H, int W, float eps, int apply_instance_norm, float* out, void* stream);
/* FABlock2D axis pooling of the normalised input: x [B,C,H,W] device, sample b at x + b * x_bs floats (x_bs >= C*H*W);
 * ss [B][C][2] device = per (sample, channel) (scale, shift), or null = identity:
 *   mx [B,H,C] = scale * mean_W(x) + shift,  my [B,W,C] = scale * mean_H(x) + shift.
 * The order of every sum is a function of (H, W) only: a sample's result does not depend on B. */
int lns_op_fa_pool(const float* x, int64_t x_bs, const float* ss, int B, int C, int H, int W,
                   float* mx, float* my, void* stream);

/* FourierBasicBlock (modules/basics.py:531-583) and CondFourierBasicBlock
 * (modules/fourier_cond.py:84-117) as standalone ops (not reached by any shipped config):
 *   y = [x +] act( irfft2(modes(rfft2(x)) . W{1,2} [* FreqLinear(cond)]) + conv1x1(x) [+ Linear(cond)] )
 * x [B,Cin,H,W], y [B,Cout,H,W] device; all weights HOST pointers in the reference's state_dict layout:
 *   w1,w2 [Cin,Cout,m1,m2,2]; conv_w [Cout,Cin,1,1], conv_b [Cout];
 *   conditional only (cond != NULL, device [B,Cin]): freq_w [Cin,4*m1*m2], freq_b [1,4*m1*m2], lin_w [Cout,Cin], lin_b [Cout].
 * activation: 1 silu, 2 gelu, 3 relu, 4 tanh, 5 sigmoid (ACTIVATION_REGISTRY, basics.py:10-16; the conditional block
 * hard-codes GELU, fourier_cond.py:114); residual != 0 adds x (needs Cin == Cout, basics.py:581-582). */
int lns_op_fourier_block(const float* x, int B, int Cin, int Cout, int H, int W, int m1, int m2, const float* w1_host,
                         const float* w2_host, const float* conv_w_host, const float* conv_b_host,
                         const float* cond, const float* freq_w_host, const float* freq_b_host,
                         const float* lin_w_host, const float* lin_b_host, int activation, int residual,
                         float* y, void* stream);

/* The same block as an object with DEVICE-RESIDENT weights: what a module instance (FourierBasicBlock.forward,
 * modules/basics.py:574-583; CondFourierBasicBlock.forward, modules/fourier_cond.py:106-117) calls on every forward.
 * create uploads the weights once (host pointers as above; freq_w_host == NULL: the unconditional block) onto HIP device
 * `device`; forward only launches (asynchronous on `stream`; the scratch buffer grows when a larger shape arrives);
 * cond must be given exactly when the block is conditional. */
typedef struct lns_fourier_block lns_fourier_block;
int lns_fourier_block_create(int Cin, int Cout, int m1, int m2, const float* w1_host, const float* w2_host,
                             const float* conv_w_host, const float* conv_b_host, const float* freq_w_host,
                             const float* freq_b_host, const float* lin_w_host, const float* lin_b_host, int activation,
                             int residual, int device, lns_fourier_block** out);
int lns_fourier_block_forward(lns_fourier_block* h, const float* x, const float* cond, int B, int H, int W, float* y,
                              void* stream);
void lns_fourier_block_destroy(lns_fourier_block* h);

/* ---- "next row" (SURVEY 8f-2): the step right after the path -------------------------------------------------
 * Fused denormalise + relative-L2 metric of a decoded rollout against the ground truth, one pass over both tensors:
 *   yd = y*std + mean (dataset/ns2d_fno_stage2_simpleae.py:140-149), err = sqrt(sum (yhat_d - y_d)^2 / max(sum y_d^2, eps))
 *   frame-wise over (H,W)   -> frame_out [B,T,C]   (relative_lp_loss(reduce_dim=(3,4)), training_utils.py:9-23,
 *   sequence-wise over (T,H,W) -> seq_out [B,C]     (reduce_dim=(1,3,4)),                train_stage2_ns2d.py:254-257)
 * yhat, y [B,T,C,H,W] device fp32 (normalised); scratch: device, >= B*T*C*2 floats; either output may be NULL. */
int lns_metric_rel_l2(const float* yhat, const float* y, int B, int T, int C, int HW, float mean, float std, float eps,
                      float* frame_out, float* seq_out, float* scratch, void* stream);

/* Same metric with per-channel statistics and the boundary handling of the other datasets' denormalize():
 *   v = x*std[c] + mean[c]                     (dataset/Stage2_SW.py:60-72, per-channel u / v / pres stats)
 *   flags[c] & LNS_METRIC_ZERO_WALLS: first/last row and column set to 0 after the affine map
 *                                              (closed-tank velocities, dataset/twophase_flow_stage2.py:370-383)
 *   flags[c] & LNS_METRIC_CLAMP:      v clamped to [clamp_lo, clamp_hi]   (VOF channel, :388, [0, 1+1e-8])
 * applied to both yhat and y as train_stage2_twophase*.py:251-254 / :287-290 do.  mean/std/flags: HOST arrays of C
 * entries (NULL = 0 / 1 / 0); C <= 8. */
#define LNS_METRIC_ZERO_WALLS 1
#define LNS_METRIC_CLAMP 2
int lns_metric_rel_l2_ch(const float* yhat, const float* y, int B, int T, int C, int H, int W, const float* mean_host,
                         const float* std_host, const int* flags_host, float clamp_lo, float clamp_hi, float eps,
                         float* frame_out, float* seq_out, float* scratch, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LNS_H_ */

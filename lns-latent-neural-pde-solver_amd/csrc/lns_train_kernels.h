// Kernels of the latent training rollout's backward pass (lns_train_kernels.hip).  All tensors fp32 NCHW.
#pragma once
#include <hip/hip_runtime.h>

namespace lns {

// OIHW weight -> [tap][Cin_pad][Cout_pad] pack of the fp32 convolution kernels; transpose_flip = 1: the pack of the
// data-gradient convolution (channels swapped, taps mirrored; pads given for THAT convolution: Cin_pad >= Cout, ...)
hipError_t launch_pack_conv_w(const float* w, float* dst, int Cout, int Cin, int k, int Cin_pad, int Cout_pad, int transpose_flip,
                              hipStream_t s);

struct GnTrainArgs {
    const float* x; float* y;          // forward: y = GN(x)
    float* stats;                      // [B][groups][2] (mean, rstd): written by forward, read by backward
    const float* gamma; const float* beta;
    const float* dy; float* dx;        // backward
    const float* add;                  // backward: dx = add + ...  (gradient arriving over the skip connection) or null
    float* part;                       // backward: [B][C][2] per-sample (dgamma, dbeta) partials
    int B, C, HW, groups; float eps;
};
hipError_t launch_gn_train_fwd(const GnTrainArgs& a, hipStream_t s);
hipError_t launch_gn_train_bwd(const GnTrainArgs& a, hipStream_t s);
hipError_t launch_colsum2(const float* part, int B, int C, float* dst_a, float* dst_b, int accumulate, hipStream_t s);

hipError_t launch_gelu_fwd(const float* u, float* y, long n, hipStream_t s);
hipError_t launch_gelu_bwd(const float* dy, const float* u, float* du, long n, hipStream_t s);
hipError_t launch_add(const float* a, const float* b, float* y, long n, hipStream_t s);
hipError_t launch_add_rows(const float* a, long sa, const float* b, long sb, float* y, long sy, int rows, long n, hipStream_t s);
hipError_t launch_bias_grad(const float* dy, int B, int C, int HW, float* db, int accumulate, hipStream_t s);

struct WgradArgs {
    const float* dy;                   // [B][Cout][H][W]
    const float* x;                    // [B][Cin][H][W]
    const int* rowmap; const int* colmap;   // padded coordinate -> source row / column or -1 (H + (k-1) dil entries)
    float* dw;                         // [Cout][Cin][k][k] (OIHW, the parameter's own layout)
    int B, Cin, Cout, H, W, k, dil, accumulate;
    // batch-parallel form only (wgrad_split.inc); launch_conv_wgrad reads none of these
    long x_bs;                         // floats between two samples of x (Cin*H*W, or T*c*H*W for a view of z_pred)
    float* part;                       // [S][Cout][Cin][k*k] partial sums
    int S;                             // slices = wgrad_split_slices(B, H, W, Cin, Cout, k)
    int cps, nchunk, patch_pos;        // filled by the launcher
};
hipError_t launch_conv_wgrad(const WgradArgs& a, hipStream_t s);
// Batch-parallel form: K = (sample, 64-pixel chunk) cut into S slices, one block per (co tile, ci tile, slice) writes a
// partial tile, wgrad_reduce_kernel sums them in ascending slice order (and adds dw when a.accumulate).  Host helpers need no device.
int wgrad_split_slices(int B, int H, int W, int Cin, int Cout, int k);
size_t wgrad_split_scratch_floats(int B, int H, int W, int Cin, int Cout, int k);
hipError_t init_train_kernels();       // dynamic-LDS attributes of the batch-parallel kernels; needs a GPU
hipError_t launch_conv_wgrad_split(const WgradArgs& a, hipStream_t s);

// conditional propagator: per-channel reductions / modulation of fields, per-sample vector network (one block each)
hipError_t launch_chan_dot(const float* a, const float* b2, float* out, int BC, int HW, int accumulate, hipStream_t s);
hipError_t launch_chan_scale(const float* x, const float* m, const float* add, float* y, int BC, int HW, hipStream_t s);
hipError_t launch_vec_fourier(const float* param, float* out, int B, int E, hipStream_t s);
hipError_t launch_vec_linear_fwd(const float* x, const float* W, const float* bias, float* y, int B, int I, int O, hipStream_t s);
// dx, dW, db: each nullable (a null output is not computed)
hipError_t launch_vec_linear_bwd(const float* dy, const float* x, const float* W, float* dx, int dx_acc, float* dW, float* db, int p_acc,
                                 int B, int I, int O, hipStream_t s);
hipError_t launch_vec_gelu(const float* u, const float* dy, float* out, int n, hipStream_t s);
hipError_t launch_vec_gn(const float* x, const float* gamma, const float* beta, float* y, float* stats, const float* dy, float* dx,
                         float* dgamma, float* dbeta, int p_acc, int B, int D, float eps, hipStream_t s);
// (backward: dgamma / dbeta null = the state-only adjoint, dx alone)

// ---- latent fit (latent_fit.inc) ---------------------------------------------------------------------------------------
// d loss / d param of the conditional propagator from d fe [B][E] and the forward's fe = [cos | sin] (one thread per sample)
hipError_t launch_vec_fourier_bwd(const float* fe, const float* dfe, float* grad_param, int B, int E, hipStream_t s);
// Observation loss of a rollout, per trajectory.  The table is a kernel argument: steps ascending, coef[k] = (float)(2 w_k / n),
// coef_bg = (float)(2 lambda / n), the weights themselves and 1 / n in double for the finishing sum.
constexpr int OBS_MAX = 64;
struct ObsTable {
    int n_obs, has_bg;
    int steps[OBS_MAX];
    float coef[OBS_MAX];
    float coef_bg, pad;
    double weight[OBS_MAX];
    double lambda, inv_n;
};
// z_pred [B][T][n], obs [B][n_obs][n], z0 / zb [B][n] (read when tb.has_bg) -> per [B][n_obs] (nullable), loss [B],
// grad [B][T][n] (zeros on steps that are not observed), gbg [B][n] (nullable); part: B * (n_obs + 1) doubles.
hipError_t launch_obs_mse(const ObsTable& tb, const float* z_pred, const float* obs, const float* z0, const float* zb, int B, int T,
                          long n, float* per, float* loss, float* grad, float* gbg, double* part, hipStream_t s);

// ---- Gauss-Newton latent fit (fit_gn.inc) ---------------------------------------------------------------------------------
// The observation table of a Gauss-Newton product as a kernel argument: coef[k] = (float)(2 w_k / n) as in ObsTable,
// cw[k] = 2 w_k / n and cd = 2 lambda / n + mu in double (the sums of v^T H v), c_d = (float)cd (the diagonal term of H v).
struct GnTable {
    int n_obs, pad;
    int steps[OBS_MAX];
    float coef[OBS_MAX];
    float c_d, pad2;
    double cw[OBS_MAX];
    double cd;
};
// jv [B][T][n] in place: part[b][k] = sum_i (double)jv[b,t_k,i]^2 on the unscaled values, then jv = coef[k] jv; exact zeros on
// the steps that are not observed; part[b][n_obs] = sum_i (double)v[b,i]^2.  part: B * (n_obs + 1) doubles.
hipError_t launch_gn_weight(const GnTable& tb, float* jv, const float* v, int B, int T, long n, double* part, hipStream_t s);
// vhv[b] (nullable) = sum_k cw[k] part[b][k] + cd part[b][n_obs] in double; hv[i] = hv[i] + c_d v[i] in fp32 when c_d != 0
hipError_t launch_gn_finish(const GnTable& tb, const double* part, float* hv, const float* v, int B, long n, double* vhv, hipStream_t s);
// Conjugate gradients per sample on [B][n] vectors, one block per sample, scalars rs / rs0 [B] in double on the device.
// start: x = 0, r = p = -g, rs = rs0 = <r, r>.  update: one step with <p, H p> = php[b] (php null: <p, hp> summed here); a
// sample with rs or php not finite or not positive, or rs <= tol2 rs0, is not written at all.  applied [B] (nullable): += 1.
hipError_t launch_cg_start(const float* g, float* x, float* r, float* p, int B, long n, double* rs, double* rs0, hipStream_t s);
hipError_t launch_cg_update(float* x, float* r, float* p, const float* hp, const double* php, int B, long n, double tol2, double* rs,
                            const double* rs0, int* applied, hipStream_t s);
// resid[b] = (float)sqrt(rs / rs0), 0 where rs0 is 0
hipError_t launch_cg_resid(const double* rs, const double* rs0, int B, float* resid, hipStream_t s);

// ---- tangent-linear rollout (tangent.inc) --------------------------------------------------------------------------------
// Tangent tensors are [B*K][C][HW], row r = b*K + k; what is read from the forward's tape belongs to sample b = r / K.
struct GnJvpArgs {
    const float* x;                    // tape: the GroupNorm's input [B][C][HW]
    const float* stats;                // tape: [B][groups][2] (mean, rstd)
    const float* gamma;
    const float* dx; float* dy;        // [B*K][C][HW]: dy = gamma rstd (dx - mean_g(dx) - xh mean_g(dx xh)) [+ add]
    const float* add;                  // [B*K][C][HW] or null
    int B, K, C, HW, groups;
};
hipError_t launch_gn_train_jvp(const GnJvpArgs& a, hipStream_t s);
// da[r][i] = du[r][i] gelu'(u[r / K][i]); n: elements of one sample; da may be du
hipError_t launch_gelu_jvp(const float* du, const float* u, float* da, int rows, int K, long n, hipStream_t s);
// dxm[r][c][p] = dx1[r][c][p] (1 + m[r / K][c])
hipError_t launch_chan_scale_rows(const float* dx1, const float* m, float* dxm, int rows, int K, int C, int HW, hipStream_t s);
// One pass of modified Gram-Schmidt over the K vectors of every sample, V [B][K][n] in place, sums in double in
// obs_mse_kernel's order.  R [B][K][K] (upper triangle, zeros below) and logr_acc [B][K] (+= log R_kk) are nullable.
hipError_t launch_orthonormalize(float* V, int B, int K, long n, double* R, double* logr_acc, hipStream_t s);

// ---- loss and optimiser of the training step (lns_optim.inc) ----------------------------------------------------------
// F.smooth_l1_loss(pred, target, 'mean', beta) -> *loss_out (device float) and, if grad != null, dL/dpred, in one pass.
// partial: device scratch of smooth_l1_partials(n) floats (one per SL1_CHUNK elements).  n >= 1, beta > 0.
constexpr int SL1_CHUNK = 4096;
long smooth_l1_partials(long n);
hipError_t launch_smooth_l1(const float* pred, const float* target, long n, float beta, float* loss_out, float* grad, float* partial,
                            hipStream_t s);

// torch.optim.Adam's update of `count` tensors, ADAM_MAX_TENSORS per launch (the table is a kernel argument).
constexpr int ADAM_MAX_TENSORS = 96;
struct AdamTensor { float* p; const float* g; float* m; float* v; unsigned n; unsigned first; };
struct AdamScalars { float step_size, beta1, one_minus_beta1, beta2, one_minus_beta2, bc2_sqrt, eps, weight_decay; };
hipError_t launch_adam_multi(AdamTensor* tensors, int count, const AdamScalars& sc, hipStream_t s);

// clip_grad_norm_'s global L2 norm (double partials, one per 2048-element chunk of a tensor, fixed summation order) and
// clip coefficient of `count` gradient tensors as device floats; the update on the clipped gradient (Adam or AdamW).
struct NormTensor { const float* g; unsigned n; unsigned first; };
long grad_norm_partials(const NormTensor* tensors, int count);
hipError_t launch_grad_norm(const NormTensor* tensors, int count, float max_norm, int skip_nonfinite, float* norm_out, float* coef_out,
                            unsigned* skipped, double* partial, hipStream_t s);
hipError_t launch_grad_scale(const NormTensor* tensors, int count, const float* coef, hipStream_t s);
hipError_t launch_update_multi(AdamTensor* tensors, int count, const AdamScalars& sc, const float* coef, int decoupled, float decay,
                               hipStream_t s);

}  // namespace lns

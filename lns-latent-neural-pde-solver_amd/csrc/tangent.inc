// ---------------------------------------------------------------------------------------------------------------------
// Kernels of the tangent-linear rollout  (included by lns_train_kernels.hip; include/lns.h "tangent-linear rollout")
//
// No reference counterpart: the reference never linearises its propagator.  What is stated here is the forward-mode chain
// rule of the training forward's own text (lns_train.inc), evaluated on that call's tape.  K tangents of every sample ride
// the batch axis: a tangent tensor is [B*K][C][HW] with row r = b*K + k, and everything read from the tape ([B][C][HW],
// GroupNorm statistics, the conditional propagator's m) belongs to sample b = r / K.  A convolution is linear, so its
// tangent is the forward convolution itself (conv_mfma_kernel, no bias) and needs nothing here; the parts that are not
// convolutions are:
//   * gn_train_jvp_kernel: dy = gamma rstd (dx - mean_g(dx) - xh mean_g(dx xh)) [+ add] -- gn_train_bwd_kernel's operator
//     (the Jacobian of the normalisation is symmetric) with gamma applied after the projection instead of before it;
//   * gelu_jvp_kernel, chan_scale_rows_kernel: elementwise with the row map;
//   * orthonormalize_kernel: one pass of modified Gram-Schmidt over the K tangents of a sample, sums in double.
// All sums have one fixed order; no atomics; scalar accesses only (the bits do not depend on the pointers' alignment).
// ---------------------------------------------------------------------------------------------------------------------

// One block per (group, row).  dx, the mean and the product dx xh are ROUNDED fp32 values in both loops (fp contract off):
// the mean that is subtracted is the mean of the very values it is subtracted from, and where a group holds a single value
// dx - mean_g(dx) is exactly 0 (and xh is: the tape's mean is that value).
__global__ __launch_bounds__(256) void gn_train_jvp_kernel(GnJvpArgs a) {
#pragma clang fp contract(off)
    __shared__ float red[4];
    const int g = blockIdx.x, r = blockIdx.y, b = r / a.K, cg = a.C / a.groups;
    const long n = (long)cg * a.HW;
    const long base = ((long)r * a.C + (long)g * cg) * a.HW;
    const float* x = a.x + ((long)b * a.C + (long)g * cg) * a.HW;
    const float* dx = a.dx + base;
    const float mean = a.stats[((long)b * a.groups + g) * 2], rstd = a.stats[((long)b * a.groups + g) * 2 + 1];
    float s1 = 0.0f, s2 = 0.0f;
    for (long i = threadIdx.x; i < n; i += 256) {
        const float xh = (x[i] - mean) * rstd, d = dx[i];
        s1 += d; s2 += d * xh;
    }
    const float m1 = t_block_sum(s1, red) / (float)n;
    const float m2 = t_block_sum(s2, red) / (float)n;
    float* dy = a.dy + base;
    const float* add = a.add ? a.add + base : nullptr;
    for (long i = threadIdx.x; i < n; i += 256) {
        const int c = g * cg + (int)(i / a.HW);
        const float xh = (x[i] - mean) * rstd;
        const float v = a.gamma[c] * rstd * (dx[i] - m1 - xh * m2);
        dy[i] = add ? add[i] + v : v;
    }
}
hipError_t launch_gn_train_jvp(const GnJvpArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(gn_train_jvp_kernel, dim3(a.groups, a.B * a.K), dim3(256), 0, s, a);
    return hipGetLastError();
}

// da[r][i] = du[r][i] gelu'(u[r / K][i]), the derivative as gelu_bwd_kernel writes it; n: elements of one sample.
// da may be du (each element is read before it is written, by the same thread).
__global__ __launch_bounds__(256) void gelu_jvp_kernel(const float* du, const float* u, float* da, int K, long n) {
    const int r = blockIdx.y, b = r / K;
    const float* ub = u + (long)b * n;
    const float* dur = du + (long)r * n;
    float* dar = da + (long)r * n;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const float v = ub[i];
        const float cdf = 0.5f * (1.0f + erff(v * 0.70710678118654752440f));
        const float pdf = 0.39894228040143267794f * expf(-0.5f * v * v);
        dar[i] = dur[i] * (cdf + v * pdf);
    }
}
hipError_t launch_gelu_jvp(const float* du, const float* u, float* da, int rows, int K, long n, hipStream_t s) {
    hipLaunchKernelGGL(gelu_jvp_kernel, dim3(ew_blocks(n), rows), dim3(256), 0, s, du, u, da, K, n);
    return hipGetLastError();
}

// dxm[r][c][p] = dx1[r][c][p] (1 + m[r / K][c])      (conditional propagator: m does not depend on the state)
__global__ __launch_bounds__(256) void chan_scale_rows_kernel(const float* dx1, const float* m, float* dxm, int K, int C, int HW) {
    const int r = blockIdx.y, b = r / K;
    const long n = (long)C * HW;
    const float* mb = m + (long)b * C;
    const float* xr = dx1 + (long)r * n;
    float* yr = dxm + (long)r * n;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) yr[i] = xr[i] * (1.0f + mb[i / HW]);
}
hipError_t launch_chan_scale_rows(const float* dx1, const float* m, float* dxm, int rows, int K, int C, int HW, hipStream_t s) {
    hipLaunchKernelGGL(chan_scale_rows_kernel, dim3(ew_blocks((long)C * HW), rows), dim3(256), 0, s, dx1, m, dxm, K, C, HW);
    return hipGetLastError();
}

// ---- orthonormalisation ---------------------------------------------------------------------------------------------
// sum over the block of a double, the order of obs_mse_kernel: the wave by obs_wave_sum (a butterfly, neighbours first), the
// four waves as (w0 + w1) + (w2 + w3); the same value in every thread.  Two barriers: `red` is free again on return.
__device__ __forceinline__ double orth_block_sum(double v, double* red) {
    v = obs_wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const double s = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
    return s;
}

// One block per sample, V [B][K][n] in place: for k ascending, for j < k ascending r_jk = <q_j, v_k> and
// v_k[i] = (float)((double)v_k[i] - r_jk (double)q_j[i]) (the v_k of the inner product is the one the earlier projections
// left: modified Gram-Schmidt); then R_kk = sqrt(<v_k, v_k>) and q_k[i] = (float)((double)v_k[i] / R_kk), or 0 when R_kk
// is 0.  Products and sums in double (the product of two floats is exact there); a thread takes i = tid, tid + 256, ...
// ascending and only ever touches those elements, so no thread reads what another wrote.
__global__ __launch_bounds__(256) void orthonormalize_kernel(float* __restrict__ V, int K, long n, double* __restrict__ R,
                                                             double* __restrict__ logr_acc) {
    __shared__ double red[4];
    const int b = blockIdx.x;
    float* Vb = V + (long)b * K * n;
    double* Rb = R ? R + (long)b * K * K : nullptr;
    for (int k = 0; k < K; ++k) {
        float* vk = Vb + (long)k * n;
        for (int j = 0; j < k; ++j) {
            const float* qj = Vb + (long)j * n;
            double acc = 0.0;
            for (long i = threadIdx.x; i < n; i += 256) acc += (double)qj[i] * (double)vk[i];
            const double rjk = orth_block_sum(acc, red);
            for (long i = threadIdx.x; i < n; i += 256) vk[i] = (float)((double)vk[i] - rjk * (double)qj[i]);
            if (Rb && threadIdx.x == 0) { Rb[(long)j * K + k] = rjk; Rb[(long)k * K + j] = 0.0; }
        }
        double acc = 0.0;
        for (long i = threadIdx.x; i < n; i += 256) acc += (double)vk[i] * (double)vk[i];
        const double rkk = sqrt(orth_block_sum(acc, red));
        for (long i = threadIdx.x; i < n; i += 256) vk[i] = rkk == 0.0 ? 0.0f : (float)((double)vk[i] / rkk);
        if (threadIdx.x == 0) {
            if (Rb) Rb[(long)k * K + k] = rkk;
            if (logr_acc) logr_acc[(long)b * K + k] += log(rkk);
        }
    }
}
hipError_t launch_orthonormalize(float* V, int B, int K, long n, double* R, double* logr_acc, hipStream_t s) {
    hipLaunchKernelGGL(orthonormalize_kernel, dim3(B), dim3(256), 0, s, V, K, n, R, logr_acc);
    return hipGetLastError();
}

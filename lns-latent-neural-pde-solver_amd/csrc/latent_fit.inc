// ---------------------------------------------------------------------------------------------------------------------
// Kernels of the latent state / parameter fit  (included by lns_train_kernels.hip; include/lns.h "latent fit")
//
// No reference counterpart: the reference trains the propagator and never runs it backwards onto data.  What is stated here
// is the chain rule of its own text:
//   * vec_fourier_bwd_kernel: fourier_embedding(param, E) (modules/cond_utils.py:19-38) is fe = [cos(a_k) | sin(a_k)],
//     a_k = param f_k, so d fe / d param = f_k [-sin(a_k) | cos(a_k)].  The forward's fe is still in the workspace when the
//     backward runs (the tape of the vector network), and it IS [cos | sin]: the kernel reads it instead of calling cosf /
//     sinf again -- the same fp32 values, and the backward call needs no `param` argument.
//   * obs_mse_kernel / obs_mse_finish_kernel: per trajectory, sum_k w_k mean_i (z_pred[b, t_k, i] - obs[b, k, i])^2 plus an
//     optional background term lambda mean_i (z0 - z_b)_i^2, and the gradients of both.  The observation table (steps,
//     coefficients, weights) travels in the kernel-argument block, as adam_multi_kernel's tensor table does.
// All sums have one fixed order; no atomics.
// ---------------------------------------------------------------------------------------------------------------------

// grad_param[b] = sum_k f_k (-sin(a_k) dfe[b][k] + cos(a_k) dfe[b][half + k]), k ascending, one thread per sample; f_k as
// vec_fourier_kernel computes it; dfe of the zero column of an odd E is not read.  fe: the forward's [cos | sin].
__global__ __launch_bounds__(256) void vec_fourier_bwd_kernel(const float* fe, const float* dfe, float* grad_param, int B, int E) {
    const int half = E / 2;
    for (int b = threadIdx.x; b < B; b += 256) {
        const float* f_ = fe + (long)b * E;
        const float* d_ = dfe + (long)b * E;
        float s = 0.0f;
        for (int k = 0; k < half; ++k) {
            const float f = expf(-9.210340371976184f * (float)k / (float)half);
            s += f * (f_[k] * d_[half + k] - f_[half + k] * d_[k]);
        }
        grad_param[b] = s;
    }
}
hipError_t launch_vec_fourier_bwd(const float* fe, const float* dfe, float* grad_param, int B, int E, hipStream_t s) {
    hipLaunchKernelGGL(vec_fourier_bwd_kernel, dim3(1), dim3(256), 0, s, fe, dfe, grad_param, B, E);
    return hipGetLastError();
}

// ---- observation loss ---------------------------------------------------------------------------------------------
static_assert(sizeof(ObsTable) <= 4096 - 128, "kernel-argument block limit");

__device__ __forceinline__ double obs_wave_sum(double v) {          // fixed order; the same value in every lane
    for (int m = 1; m < 64; m <<= 1) v = v + __shfl_xor(v, m, 64);
    return v;
}

// the difference and the gradient: one fp32 subtraction, one fp32 multiplication, never contracted (there is nothing to
// contract a subtraction feeding a product into, the pragma says so to the reader and to a later compiler)
__device__ __forceinline__ float obs_grad(float d, float coef) {
#pragma clang fp contract(off)
    return coef * d;
}

// grid (T + has_bg, B), 256 threads: block (t, b) owns the plane z_pred[b, t, :] -- observed: gradient and the double sum
// of squares -> part[b][k]; not observed: zeros -- and block (T, b) the background term -> part[b][n_obs].
// A thread walks its elements in ascending order (stride 256), the wave is summed by obs_wave_sum, the four waves as
// (w0 + w1) + (w2 + w3).  Scalar accesses: the bits do not depend on the pointers' alignment.
__global__ __launch_bounds__(256) void obs_mse_kernel(const ObsTable tb, const float* __restrict__ z_pred, const float* __restrict__ obs,
                                                      const float* __restrict__ z0, const float* __restrict__ zb, int T, long n,
                                                      float* __restrict__ grad, float* __restrict__ gbg, double* __restrict__ part) {
    __shared__ double red[4];
    const int t = blockIdx.x, b = blockIdx.y;
    const float* a; const float* r; float* g; float coef; int slot;
    if (t < T) {
        int k = -1;
        for (int j = 0; j < tb.n_obs; ++j) if (tb.steps[j] == t) k = j;       // uniform over the block
        g = grad + ((long)b * T + t) * n;
        if (k < 0) {
            for (long i = threadIdx.x; i < n; i += 256) g[i] = 0.0f;
            return;
        }
        a = z_pred + ((long)b * T + t) * n;
        r = obs + ((long)b * tb.n_obs + k) * n;
        coef = tb.coef[k]; slot = k;
    } else {
        a = z0 + (long)b * n; r = zb + (long)b * n;
        g = gbg ? gbg + (long)b * n : nullptr;
        coef = tb.coef_bg; slot = tb.n_obs;
    }
    double acc = 0.0;
    for (long i = threadIdx.x; i < n; i += 256) {
        const float d = a[i] - r[i];
        if (g) g[i] = obs_grad(d, coef);
        acc += (double)d * (double)d;
    }
    acc = obs_wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[(long)b * (tb.n_obs + 1) + slot] = (red[0] + red[1]) + (red[2] + red[3]);
}

// one thread per sample: the terms in ascending k in double, rounded once
__global__ __launch_bounds__(256) void obs_mse_finish_kernel(const ObsTable tb, const double* __restrict__ part, int B,
                                                             float* __restrict__ per, float* __restrict__ loss) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const double* p = part + (long)b * (tb.n_obs + 1);
    double s = 0.0;
    for (int k = 0; k < tb.n_obs; ++k) {
        const double m = p[k] * tb.inv_n;
        if (per) per[(long)b * tb.n_obs + k] = (float)m;
        s += tb.weight[k] * m;
    }
    if (tb.has_bg) s += tb.lambda * (p[tb.n_obs] * tb.inv_n);
    loss[b] = (float)s;
}

hipError_t launch_obs_mse(const ObsTable& tb, const float* z_pred, const float* obs, const float* z0, const float* zb, int B, int T,
                          long n, float* per, float* loss, float* grad, float* gbg, double* part, hipStream_t s) {
    hipLaunchKernelGGL(obs_mse_kernel, dim3(T + (tb.has_bg ? 1 : 0), B), dim3(256), 0, s, tb, z_pred, obs, z0, zb, T, n, grad, gbg, part);
    hipError_t rc = hipGetLastError();
    if (rc != hipSuccess) return rc;
    hipLaunchKernelGGL(obs_mse_finish_kernel, dim3((B + 255) / 256), dim3(256), 0, s, tb, part, B, per, loss);
    return hipGetLastError();
}

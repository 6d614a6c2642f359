// ---------------------------------------------------------------------------------------------------------------------
// Kernels of the Gauss-Newton latent fit  (included by lns_train_kernels.hip; include/lns.h "latent fit: Gauss-Newton")
//
// No reference counterpart.  The Gauss-Newton operator of the observation loss (latent_fit.inc) is
//     H v = sum_k (2 w_k / n) J_k^T (J_k v) + (2 lambda / n + mu) v,        J_k = d z_pred[t_k] / d z0,
// and both heavy halves exist: lns_train_tangent gives J v at every step, the state-only adjoint gives J^T w.  What is here
// is what stands between and around them:
//   * gn_weight_kernel: the tangent's [B][T][n] output becomes the adjoint's cotangent in place (c_k J_k v on observed
//     steps, exact zeros elsewhere) and leaves the double sums |J_k v|^2 and |v|^2, so that v^T H v is formed from the
//     tangent side alone (a sum of squares: never negative, whatever rounding the adjoint adds);
//   * gn_vhv_kernel / gn_axpy_kernel: v^T H v per sample, and the diagonal term of H v;
//   * cg_start_kernel / cg_update_kernel: conjugate gradients per sample, every scalar in double on the device.
// Order of every sum: obs_mse_kernel's (a thread adds i = tid, tid + 256, ... ascending in double, the wave by
// obs_wave_sum, the four waves as (w0 + w1) + (w2 + w3)).  No atomics; scalar accesses only.
// ---------------------------------------------------------------------------------------------------------------------
static_assert(sizeof(GnTable) <= 4096 - 128, "kernel-argument block limit");

// grid (T + 1, B): block (t, b), t < T, owns jv[b, t, :]; block (T, b) sums v[b, :]^2 -> part[b][n_obs]
__global__ __launch_bounds__(256) void gn_weight_kernel(const GnTable tb, float* __restrict__ jv, const float* __restrict__ v, int T,
                                                        long n, double* __restrict__ part) {
#pragma clang fp contract(off)
    __shared__ double red[4];
    const int t = blockIdx.x, b = blockIdx.y;
    int slot = tb.n_obs;
    double acc = 0.0;
    if (t < T) {
        int k = -1;
        for (int j = 0; j < tb.n_obs; ++j) if (tb.steps[j] == t) k = j;       // uniform over the block
        float* a = jv + ((long)b * T + t) * n;
        if (k < 0) {
            for (long i = threadIdx.x; i < n; i += 256) a[i] = 0.0f;
            return;
        }
        const float coef = tb.coef[k];
        slot = k;
        for (long i = threadIdx.x; i < n; i += 256) {
            const float x = a[i];
            acc += (double)x * (double)x;                                      // the unscaled value
            a[i] = coef * x;
        }
    } else {
        const float* a = v + (long)b * n;
        for (long i = threadIdx.x; i < n; i += 256) acc += (double)a[i] * (double)a[i];
    }
    acc = orth_block_sum(acc, red);
    if (threadIdx.x == 0) part[(long)b * (tb.n_obs + 1) + slot] = acc;
}

// one thread per sample: sum_k cw[k] part[b][k] in ascending k, the diagonal term last, all in double
__global__ __launch_bounds__(256) void gn_vhv_kernel(const GnTable tb, const double* __restrict__ part, int B, double* __restrict__ vhv) {
#pragma clang fp contract(off)
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const double* p = part + (long)b * (tb.n_obs + 1);
    double s = 0.0;
    for (int k = 0; k < tb.n_obs; ++k) s += tb.cw[k] * p[k];
    s += tb.cd * p[tb.n_obs];
    vhv[b] = s;
}

// hv[i] = hv[i] + c v[i]: one fp32 multiplication, one fp32 addition
__global__ __launch_bounds__(256) void gn_axpy_kernel(float* __restrict__ hv, const float* __restrict__ v, float c, long n) {
#pragma clang fp contract(off)
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const float cv = c * v[i];
        hv[i] = hv[i] + cv;
    }
}

hipError_t launch_gn_weight(const GnTable& tb, float* jv, const float* v, int B, int T, long n, double* part, hipStream_t s) {
    hipLaunchKernelGGL(gn_weight_kernel, dim3(T + 1, B), dim3(256), 0, s, tb, jv, v, T, n, part);
    return hipGetLastError();
}
hipError_t launch_gn_finish(const GnTable& tb, const double* part, float* hv, const float* v, int B, long n, double* vhv, hipStream_t s) {
    if (vhv) {
        hipLaunchKernelGGL(gn_vhv_kernel, dim3((B + 255) / 256), dim3(256), 0, s, tb, part, B, vhv);
        const hipError_t rc = hipGetLastError();
        if (rc != hipSuccess) return rc;
    }
    if (tb.c_d != 0.0f) hipLaunchKernelGGL(gn_axpy_kernel, dim3(ew_blocks((long)B * n)), dim3(256), 0, s, hv, v, tb.c_d, (long)B * n);
    return hipGetLastError();
}

// ---- conjugate gradients, one block per sample ---------------------------------------------------------------------------
// x = 0, r = p = -g, rs = rs0 = <r, r>
__global__ __launch_bounds__(256) void cg_start_kernel(const float* __restrict__ g, float* __restrict__ x, float* __restrict__ r,
                                                       float* __restrict__ p, long n, double* __restrict__ rs, double* __restrict__ rs0) {
    __shared__ double red[4];
    const long o = (long)blockIdx.x * n;
    double acc = 0.0;
    for (long i = threadIdx.x; i < n; i += 256) {
        const float ri = -g[o + i];
        x[o + i] = 0.0f; r[o + i] = ri; p[o + i] = ri;
        acc += (double)ri * (double)ri;
    }
    acc = orth_block_sum(acc, red);
    if (threadIdx.x == 0) { rs[blockIdx.x] = acc; rs0[blockIdx.x] = acc; }
}

// One step.  php: the caller's <p, H p> per sample, or null: <p, hp> in the same order here.  A sample that is not active
// returns before its first store.  A thread only ever touches its own elements i = tid, tid + 256, ...; rs[b] is read by
// every thread before the first barrier and written by thread 0 after the last.
__global__ __launch_bounds__(256) void cg_update_kernel(float* __restrict__ x, float* __restrict__ r, float* __restrict__ p,
                                                        const float* __restrict__ hp, const double* __restrict__ php, long n, double tol2,
                                                        double* __restrict__ rs, const double* __restrict__ rs0, int* __restrict__ applied) {
#pragma clang fp contract(off)
    __shared__ double red[4];
    const int b = blockIdx.x;
    const long o = (long)b * n;
    const double rs_b = rs[b], rs0_b = rs0[b];
    double d;
    if (php) d = php[b];
    else {
        double acc = 0.0;
        for (long i = threadIdx.x; i < n; i += 256) acc += (double)p[o + i] * (double)hp[o + i];
        d = orth_block_sum(acc, red);
    }
    const bool active = isfinite(rs_b) && rs_b > 0.0 && isfinite(d) && d > 0.0 && rs_b > tol2 * rs0_b;      // uniform over the block
    if (!active) return;
    const double alpha = rs_b / d;
    double acc = 0.0;
    for (long i = threadIdx.x; i < n; i += 256) {
        const double ap = alpha * (double)p[o + i], ah = alpha * (double)hp[o + i];
        x[o + i] = (float)((double)x[o + i] + ap);
        const float ri = (float)((double)r[o + i] - ah);
        r[o + i] = ri;
        acc += (double)ri * (double)ri;
    }
    const double rs_new = orth_block_sum(acc, red);
    const double beta = rs_new / rs_b;
    for (long i = threadIdx.x; i < n; i += 256) {
        const double bp = beta * (double)p[o + i];
        p[o + i] = (float)((double)r[o + i] + bp);
    }
    if (threadIdx.x == 0) {
        rs[b] = rs_new;
        if (applied) applied[b] += 1;
    }
}

// resid[b] = (float)sqrt(rs / rs0), 0 where rs0 is 0; one thread per sample
__global__ __launch_bounds__(256) void cg_resid_kernel(const double* __restrict__ rs, const double* __restrict__ rs0, int B,
                                                       float* __restrict__ resid) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    resid[b] = rs0[b] > 0.0 ? (float)sqrt(rs[b] / rs0[b]) : 0.0f;
}

hipError_t launch_cg_start(const float* g, float* x, float* r, float* p, int B, long n, double* rs, double* rs0, hipStream_t s) {
    hipLaunchKernelGGL(cg_start_kernel, dim3(B), dim3(256), 0, s, g, x, r, p, n, rs, rs0);
    return hipGetLastError();
}
hipError_t launch_cg_update(float* x, float* r, float* p, const float* hp, const double* php, int B, long n, double tol2, double* rs,
                            const double* rs0, int* applied, hipStream_t s) {
    hipLaunchKernelGGL(cg_update_kernel, dim3(B), dim3(256), 0, s, x, r, p, hp, php, n, tol2, rs, rs0, applied);
    return hipGetLastError();
}
hipError_t launch_cg_resid(const double* rs, const double* rs0, int B, float* resid, hipStream_t s) {
    hipLaunchKernelGGL(cg_resid_kernel, dim3((B + 255) / 256), dim3(256), 0, s, rs, rs0, B, resid);
    return hipGetLastError();
}

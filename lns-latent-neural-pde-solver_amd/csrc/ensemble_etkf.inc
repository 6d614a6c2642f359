// ---- ensemble transform Kalman filter (lns_kernels.h EnsembleObsGramArgs, EtkfTransformArgs; the statement: include/lns.h) ----
// Three kernels, all arithmetic in double:
//   * ensemble_obs_gram_kernel<TS>: a block owns one slice of LNS_ETKF_SLICE values of the frame of one (b, step) and walks
//     it in chunks of 64 values.  A chunk's anomalies Y[p][m] = f_m - ybar and weighted anomalies Yw[p][m] = r_p * Y[p][m]
//     are staged in LDS (value-major rows of 16 * TS + 2 doubles: a thread's TS members are contiguous, a row starts on
//     16 bytes); thread (ti, tj) of the 16 x 16 grid owns the TS x TS tile S[ti*TS .. ][tj*TS .. ] in registers and adds
//     one fma per value, ascending; only tiles with ti <= tj work (the finish kernel mirrors).  TS = 2 serves M <= 32,
//     TS = 4 M <= 64.  An unobserved value (!(r > 0)) is never loaded: its rows are zero.  Partials go to scratch; no atomics.
//   * ensemble_obs_gram_finish_kernel: adds the slices in ascending order, mirrors the triangle.
//   * etkf_transform_kernel: one block per sample; A and Q in LDS; cyclic Jacobi in the round-robin order of include/lns.h.
//   * ensemble_transform_kernel: one thread per (b, element): its M values into its own LDS column, then the M outputs.
template <int TS>
__global__ __launch_bounds__(256) void ensemble_obs_gram_kernel(EnsembleObsGramArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int LD = 16 * TS + 2;
    double* Yw = reinterpret_cast<double*>(smem);      // [64][LD]
    double* Y = Yw + 64 * LD;                          // [64][LD]
    double* dd = Y + 64 * LD;                          // [64] y - ybar (0 where unobserved)
    double* rr = dd + 64;                              // [64] r (0 where unobserved)
    double* mu = rr + 64;                              // [64] ybar
    const int tid = threadIdx.x, M = a.M;
    const int HW = a.H * a.W;
    const long P = (long)a.C * HW;
    const int b = blockIdx.y, j = blockIdx.z;
    const long s = (long)j * a.B + b;                  // launch sample of frames [kk][B][M][P]
    const float* f = a.frames + s * M * P;
    const float* g = a.y + ((long)b * a.y_T + a.y_t + j) * P;
    const float* rv = a.rinv + (long)b * a.r_bs + (long)(a.o_t + j) * a.r_ss;
    const long p_lo = (long)blockIdx.x * LNS_ETKF_SLICE;
    const long p_hi = p_lo + LNS_ETKF_SLICE < P ? p_lo + LNS_ETKF_SLICE : P;
    for (int k = tid; k < 2 * 64 * LD; k += 256) Yw[k] = 0.0;       // (Yw and Y are adjacent; the padding columns stay zero)
    const int pl = tid & 63, mq = tid >> 6;
    const int ti = tid >> 4, tj = tid & 15;
    const bool tile = ti <= tj && ti * TS < M;
    double acc[TS][TS];
#pragma unroll
    for (int k = 0; k < TS; ++k)
#pragma unroll
        for (int l = 0; l < TS; ++l) acc[k][l] = 0.0;
    double gacc = 0.0, s_dd = 0.0, s_r = 0.0;
    int s_n = 0;
    __syncthreads();
    for (long p0 = p_lo; p0 < p_hi; p0 += 64) {
        const long p = p0 + pl;
        float r = 0.0f;
        if (p < p_hi) r = rv[p];
        const bool obs = p < p_hi && r > 0.0f;         // a select: an unobserved value contributes nothing, whatever it holds
        const int c = obs ? (int)(p / HW) : 0, i = obs ? (int)(p - (long)c * HW) : 0;
        const auto [sd, mean, lo, hi, walls, clampv] = ChannelNorm(a.norm, c);
        bool zero = false;
        if (a.denorm && walls) { const int row = i / a.W, cx = i - row * a.W; zero = row == 0 || row == a.H - 1 || cx == 0 || cx == a.W - 1; }
        for (int m = mq; m < M; m += 4) {
            double v = 0.0;
            if (obs) {
                float x = f[(long)m * P + p];
                if (a.denorm) x = score_denorm(x, sd, mean, zero, clampv, lo, hi);
                v = (double)x;
            }
            Y[pl * LD + m] = v;
        }
        __syncthreads();
        if (tid < 64) {                                // (mq == 0: obs, c, zero are those of value pl)
            double sum = Y[pl * LD];
            for (int m = 1; m < M; ++m) sum = sum + Y[pl * LD + m];
            const double yb = sum / (double)M;
            double d = 0.0;
            if (obs) {
                float q = g[p];
                if (a.denorm) q = score_denorm(q, sd, mean, zero, clampv, lo, hi);
                d = (double)q - yb;
            }
            mu[pl] = yb; dd[pl] = d; rr[pl] = obs ? (double)r : 0.0;
        }
        __syncthreads();
        for (int m = mq; m < M; m += 4) {
            const double v = Y[pl * LD + m] - mu[pl];
            Y[pl * LD + m] = v;
            Yw[pl * LD + m] = rr[pl] * v;
        }
        __syncthreads();
        if (tile) {
            for (int q = 0; q < 64; ++q) {
                double av[TS], bv[TS];
#pragma unroll
                for (int k = 0; k < TS; ++k) { av[k] = Yw[q * LD + ti * TS + k]; bv[k] = Y[q * LD + tj * TS + k]; }
#pragma unroll
                for (int k = 0; k < TS; ++k)
#pragma unroll
                    for (int l = 0; l < TS; ++l) acc[k][l] = fma(av[k], bv[l], acc[k][l]);
            }
        }
        if (tid < M)
            for (int q = 0; q < 64; ++q) gacc = fma(Yw[q * LD + tid], dd[q], gacc);
        if (tid == 255)
            for (int q = 0; q < 64; ++q)
                if (rr[q] > 0.0) { const double t = rr[q] * dd[q]; s_dd = fma(t, dd[q], s_dd); s_r = s_r + rr[q]; ++s_n; }
        __syncthreads();
    }
    const size_t E = (size_t)M * M + M + 3;
    double* out = a.part + (((size_t)b * a.o_T + a.o_t + j) * a.nsl + blockIdx.x) * E;
    if (tile) {
#pragma unroll
        for (int k = 0; k < TS; ++k)
#pragma unroll
            for (int l = 0; l < TS; ++l) {
                const int ii = ti * TS + k, jj = tj * TS + l;
                if (ii < M && jj < M) out[ii * M + jj] = acc[k][l];
            }
    }
    if (tid < M) out[M * M + tid] = gacc;
    if (tid == 255) { out[M * M + M] = s_dd; out[M * M + M + 1] = s_r; out[M * M + M + 2] = (double)s_n; }
}

__global__ __launch_bounds__(256) void ensemble_obs_gram_finish_kernel(const double* __restrict__ part, int nsl, int M, double* __restrict__ S,
                                                                       double* __restrict__ g, double* __restrict__ stat) {
#pragma clang fp contract(off)
    const int bn = blockIdx.x, MM = M * M, E = MM + M + 3;
    const double* src = part + (size_t)bn * nsl * E;
    for (int e = threadIdx.x; e < E; e += 256) {
        int from = e;
        if (e < MM) { const int i = e / M, j = e - i * M; if (i > j) from = j * M + i; }
        double v = src[from];
        for (int sl = 1; sl < nsl; ++sl) v = v + src[(size_t)sl * E + from];
        if (e < MM) S[(size_t)bn * MM + e] = v;
        else if (e < MM + M) g[(size_t)bn * M + (e - MM)] = v;
        else stat[(size_t)bn * 3 + (e - MM - M)] = v;
    }
}

hipError_t launch_ensemble_obs_gram(const EnsembleObsGramArgs& a, hipStream_t s) {
    if (a.M < 2 || a.M > LNS_ETKF_MAX_MEMBERS || a.nsl != etkf_slices((long)a.C * a.H * a.W)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)a.nsl, (unsigned)a.B, (unsigned)a.kk);
    if (a.M <= 32) {
        const size_t lds = (size_t)(2 * 64 * (16 * 2 + 2) + 3 * 64) * sizeof(double);
        hipLaunchKernelGGL(ensemble_obs_gram_kernel<2>, grid, dim3(256), lds, s, a);
    } else {
        const size_t lds = (size_t)(2 * 64 * (16 * 4 + 2) + 3 * 64) * sizeof(double);   // 69120 bytes
        hipLaunchKernelGGL(ensemble_obs_gram_kernel<4>, grid, dim3(256), lds, s, a);
    }
    return hipGetLastError();
}

hipError_t launch_ensemble_obs_gram_finish(const double* part, int BN, int nsl, int M, double* S, double* g, double* stat, hipStream_t s) {
    hipLaunchKernelGGL(ensemble_obs_gram_finish_kernel, dim3((unsigned)BN), dim3(256), 0, s, part, nsl, M, S, g, stat);
    return hipGetLastError();
}

// The pair k of round r of the round-robin order over n = M + (M & 1) indices (include/lns.h): p < q, or q >= M for the pair
// of the padding index of an odd M, which rests.
__device__ __forceinline__ void etkf_pair(int n, int r, int k, int* p, int* q) {
    int u, v;
    if (k == 0) { u = n - 1; v = r; }
    else { u = (r + k) % (n - 1); v = (r - k + n - 1) % (n - 1); }
    *p = u < v ? u : v;
    *q = u < v ? v : u;
}

__global__ __launch_bounds__(256) void etkf_transform_kernel(EtkfTransformArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int M = a.M, MM = M * M, b = blockIdx.x, tid = threadIdx.x;
    double* A = reinterpret_cast<double*>(smem);       // [M][M]
    double* Q = A + MM;                                // [M][M]
    double* gv = Q + MM;                               // [M] g_tot
    double* lam = gv + M;                              // [M] the diagonal of A after the sweeps
    double* u = lam + M;                               // [M] Q^T g_tot
    double* wb = u + M;                                // [M] wbar
    double* fk = wb + M;                               // [M] sqrt((M - 1) / lam_k)
    double* cs = fk + M;                               // [32][2] the round's rotations
    int* pq = reinterpret_cast<int*>(cs + 64);         // [32][2] the round's pairs; p < 0: the pair rests
    int* perm = pq + 64;                               // [M] eigenvalue indices in ascending order
    int* flag = perm + 64;                             // [0]: non-finite Gram, [1]: an off-diagonal entry above the threshold
    const double dg = (double)(M - 1) / a.rho;
    if (tid < 2) flag[tid] = 0;
    __syncthreads();
    bool bad = false;
    for (int e = tid; e < MM + M; e += 256) {
        const bool mat = e < MM;
        const double* src = mat ? a.S + (size_t)b * a.n * MM + e : a.g + (size_t)b * a.n * M + (e - MM);
        const size_t st = mat ? MM : M;
        double v = src[0];
        for (int t = 1; t < a.n; ++t) v = v + src[(size_t)t * st];
        if (!isfinite(v)) bad = true;
        if (mat) {
            const int i = e / M, j = e - i * M;
            A[e] = i == j ? dg + v : v;
            Q[e] = i == j ? 1.0 : 0.0;
        } else gv[e - MM] = v;
    }
    if (bad) flag[0] = 1;
    __syncthreads();
    if (flag[0]) {                                     // this sample alone: NaN everywhere, status 1
        const double nan = __builtin_nan("");
        for (int e = tid; e < MM; e += 256) a.X[(size_t)b * MM + e] = nan;
        if (tid < M) { a.wbar[(size_t)b * M + tid] = nan; a.lam[(size_t)b * M + tid] = nan; }
        if (tid == 0) a.status[b] = 1;
        return;
    }
    const int n = M + (M & 1), half = n / 2;
    const double tol = 0x1p-52;
    int status = 2;
    for (int sweep = 0; sweep <= LNS_ETKF_MAX_SWEEPS; ++sweep) {
        for (int e = tid; e < MM; e += 256) {
            const int i = e / M, j = e - i * M;
            if (i < j && !(fabs(A[e]) <= tol * sqrt(A[i * M + i] * A[j * M + j]))) flag[1] = 1;
        }
        __syncthreads();
        const bool more = flag[1] != 0;
        __syncthreads();
        if (tid == 0) flag[1] = 0;
        if (!more) { status = 0; break; }
        if (sweep == LNS_ETKF_MAX_SWEEPS) break;
        for (int r = 0; r < n - 1; ++r) {
            if (tid < half) {
                int p, q;
                etkf_pair(n, r, tid, &p, &q);
                double c = 1.0, s = 0.0;
                const double apq = q < M ? A[p * M + q] : 0.0;
                if (apq != 0.0) {
                    const double theta = (A[q * M + q] - A[p * M + p]) / (2.0 * apq);
                    const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                    c = 1.0 / sqrt(t * t + 1.0);
                    s = t * c;
                }
                if (s == 0.0) p = -1;
                pq[2 * tid] = p; pq[2 * tid + 1] = q;
                cs[2 * tid] = c; cs[2 * tid + 1] = s;
            }
            __syncthreads();
            for (int w = tid; w < half * M; w += 256) {    // rows p, q of A <- J^T A
                const int k = w / M, j = w - k * M, p = pq[2 * k], q = pq[2 * k + 1];
                if (p < 0) continue;
                const double c = cs[2 * k], s = cs[2 * k + 1], x = A[p * M + j], y = A[q * M + j];
                A[p * M + j] = c * x - s * y;
                A[q * M + j] = s * x + c * y;
            }
            __syncthreads();
            for (int w = tid; w < half * M; w += 256) {    // columns p, q of A <- A J and of Q <- Q J; a_pq = a_qp = 0
                const int k = w / M, i = w - k * M, p = pq[2 * k], q = pq[2 * k + 1];
                if (p < 0) continue;
                const double c = cs[2 * k], s = cs[2 * k + 1];
                double x = A[i * M + p], y = A[i * M + q];
                A[i * M + p] = i == q ? 0.0 : c * x - s * y;
                A[i * M + q] = i == p ? 0.0 : s * x + c * y;
                x = Q[i * M + p]; y = Q[i * M + q];
                Q[i * M + p] = c * x - s * y;
                Q[i * M + q] = s * x + c * y;
            }
            __syncthreads();
        }
    }
    if (tid < M) lam[tid] = A[tid * M + tid];
    __syncthreads();
    if (tid < M) {
        const double li = lam[tid];
        int rank = 0;
        for (int k = 0; k < M; ++k) rank += (lam[k] < li || (lam[k] == li && k < tid)) ? 1 : 0;
        perm[rank] = tid;
        double sum = 0.0;
        for (int i = 0; i < M; ++i) sum = sum + Q[i * M + tid] * gv[i];
        u[tid] = sum / li;                             // (Lambda^-1 Q^T g)_k
        fk[tid] = sqrt((double)(M - 1) / li);
    }
    __syncthreads();
    if (tid < M) {
        double sum = 0.0;
        for (int kk = 0; kk < M; ++kk) { const int k = perm[kk]; sum = sum + Q[tid * M + k] * u[k]; }
        wb[tid] = sum;
        a.wbar[(size_t)b * M + tid] = sum;
        a.lam[(size_t)b * M + tid] = lam[perm[tid]];
    }
    __syncthreads();
    for (int e = tid; e < MM; e += 256) {
        const int i = e / M, j = e - i * M;
        double t1 = 0.0, t2 = 0.0;
        for (int kk = 0; kk < M; ++kk) {
            const int k = perm[kk];
            const double qi = Q[i * M + k], qj = Q[j * M + k];
            t1 = t1 + (qi * fk[k]) * qj;
            t2 = t2 + (qj * fk[k]) * qi;
        }
        a.X[(size_t)b * MM + e] = 0.5 * (t1 + t2) + wb[i];
    }
    if (tid == 0) a.status[b] = status;
}

hipError_t launch_etkf_transform(const EtkfTransformArgs& a, hipStream_t s) {
    if (a.M < 2 || a.M > LNS_ETKF_MAX_MEMBERS || a.n < 1 || !(a.rho >= 1.0)) return hipErrorInvalidValue;
    const size_t lds = (size_t)(2 * a.M * a.M + 5 * a.M + 64) * sizeof(double) + (64 + 64 + 2) * sizeof(int);   // 69128 bytes at M = 64
    hipLaunchKernelGGL(etkf_transform_kernel, dim3((unsigned)a.B), dim3(256), lds, s, a);
    return hipGetLastError();
}

// z [B][M][n] -> out [B][M][n] (may be z): a thread owns element e of sample b, reads its M values into its LDS column
// col[k * 256 + tid] before it writes any; X[b] sits in LDS beside the columns (every lane reads the same entry).
__global__ __launch_bounds__(256) void ensemble_transform_kernel(const float* z, const double* __restrict__ X, int M, long n, float* out) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* Xs = reinterpret_cast<double*>(smem);      // [M][M]
    float* col = reinterpret_cast<float*>(Xs + M * M) + threadIdx.x;
    const int b = blockIdx.y, tid = threadIdx.x;
    for (int k = tid; k < M * M; k += 256) Xs[k] = X[(size_t)b * M * M + k];
    __syncthreads();
    const long e = (long)blockIdx.x * 256 + tid;
    if (e >= n) return;
    const float* zi = z + (long)b * M * n + e;
    float* zo = out + (long)b * M * n + e;
    double sum = 0.0;
    for (int k = 0; k < M; ++k) {
        const float v = zi[(long)k * n];
        col[k * 256] = v;
        sum = sum + (double)v;
    }
    const double zbar = sum / (double)M;
    for (int m = 0; m < M; ++m) {
        double acc = 0.0;
        for (int k = 0; k < M; ++k) {
            const double Z = (double)col[k * 256] - zbar;
            const double t = Z * Xs[k * M + m];
            acc = acc + t;
        }
        zo[(long)m * n] = (float)(zbar + acc);
    }
}

hipError_t launch_ensemble_transform(const float* z, const double* X, int B, int M, long n, float* out, hipStream_t s) {
    if (M < 2 || M > LNS_ETKF_MAX_MEMBERS || B < 1 || B > 65535 || n < 1) return hipErrorInvalidValue;
    const size_t lds = (size_t)M * M * sizeof(double) + (size_t)M * 256 * sizeof(float);   // 96 KB at M = 64
    hipLaunchKernelGGL(ensemble_transform_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)B), dim3(256), lds, s, z, X, M, n, out);
    return hipGetLastError();
}

// ---- localised ensemble transform Kalman filter (lns_kernels.h LetkfPatchGramArgs, LetkfCombineArgs, LetkfUpdateArgs; the
// statement: include/lns.h "localised ensemble transform Kalman filter") ----
// Three kernels beside those of ensemble_etkf.inc, all arithmetic in double:
//   * letkf_patch_gram_kernel<TS>: ensemble_obs_gram_kernel's register tiles (16 x 16 threads, TS x TS tiles, chunks of 64 values
//     staged in LDS, tiles with ti <= tj) with a block that owns one (patch, sample, step) and gathers the patch's values through
//     (ch, y, x).  The patch's sums go straight to part[b][step][patch], both halves of the triangle: no slices, no finish.
//   * letkf_combine_kernel: a block owns four consecutive domains of one sample (or, as a sample's last block, the global sums):
//     their tapers against the h * w patches in LDS, then every entry of S_l and g_l as the ascending sum over steps and patches,
//     unfused, each patch sum read once for the four.
//   * letkf_update_kernel: a block owns one (sample, latent pixel): X_l in LDS, the pixel's M values of up to 64 channels beside
//     it, one thread per (channel, member) output.
// The transform between them is etkf_transform_kernel as it is, one block per domain.
template <int TS>
__global__ __launch_bounds__(256) void letkf_patch_gram_kernel(LetkfPatchGramArgs a) {
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
    const int t = blockIdx.x, b = blockIdx.y, j = blockIdx.z;
    const int ty = t / a.w, tx = t - ty * a.w;
    // rows y with (y * h) / H == ty: ceil(ty * H / h) <= y < ceil((ty + 1) * H / h); the columns likewise
    const int y_lo = (int)(((long)ty * a.H + a.h - 1) / a.h), y_hi = (int)(((long)(ty + 1) * a.H + a.h - 1) / a.h);
    const int x_lo = (int)(((long)tx * a.W + a.w - 1) / a.w), x_hi = (int)(((long)(tx + 1) * a.W + a.w - 1) / a.w);
    const int nr = y_hi - y_lo, nc = x_hi - x_lo, np = nr * nc;
    const long nv = (long)a.C * np;                    // the patch's values, v = (ch * nr + row) * nc + col ascending
    const long s = (long)j * a.B + b;                  // launch sample of frames [kk][B][M][P]
    const float* f = a.frames + s * M * P;
    const float* g = a.y + ((long)b * a.y_T + a.y_t + j) * P;
    const float* rv = a.rinv + (long)b * a.r_bs + (long)(a.o_t + j) * a.r_ss;
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
    for (long v0 = 0; v0 < nv; v0 += 64) {
        const long v = v0 + pl;
        const int cnt = nv - v0 < 64 ? (int)(nv - v0) : 64;   // the rows behind cnt are zero: fma(0, 0, acc) = acc
        int c = 0, i = 0;
        long p = 0;
        if (v < nv) {
            c = (int)(v / np);
            const int rem = (int)(v - (long)c * np), row = rem / nc, col = rem - row * nc;
            i = (y_lo + row) * a.W + x_lo + col;
            p = (long)c * HW + i;
        }
        float r = 0.0f;
        if (v < nv) r = rv[p];
        const bool obs = v < nv && r > 0.0f;           // a select: an unobserved value contributes nothing, whatever it holds
        if (!obs) { c = 0; i = 0; }
        const auto [sd, mean, lo, hi, walls, clampv] = ChannelNorm(a.norm, c);
        bool zero = false;
        if (a.denorm && walls) { const int row = i / a.W, cx = i - row * a.W; zero = row == 0 || row == a.H - 1 || cx == 0 || cx == a.W - 1; }
        for (int m = mq; m < M; m += 4) {
            double val = 0.0;
            if (obs) {
                float x = f[(long)m * P + p];
                if (a.denorm) x = score_denorm(x, sd, mean, zero, clampv, lo, hi);
                val = (double)x;
            }
            Y[pl * LD + m] = val;
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
            const double val = Y[pl * LD + m] - mu[pl];
            Y[pl * LD + m] = val;
            Yw[pl * LD + m] = rr[pl] * val;
        }
        __syncthreads();
        if (tile) {
            for (int q = 0; q < cnt; ++q) {
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
            for (int q = 0; q < cnt; ++q) gacc = fma(Yw[q * LD + tid], dd[q], gacc);
        if (tid == 255)
            for (int q = 0; q < cnt; ++q)
                if (rr[q] > 0.0) { const double w = rr[q] * dd[q]; s_dd = fma(w, dd[q], s_dd); s_r = s_r + rr[q]; ++s_n; }
        __syncthreads();
    }
    const size_t E = (size_t)M * M + M + 3;
    double* out = a.part + (((size_t)b * a.o_T + a.o_t + j) * ((size_t)a.h * a.w) + t) * E;
    if (tile) {
#pragma unroll
        for (int k = 0; k < TS; ++k)
#pragma unroll
            for (int l = 0; l < TS; ++l) {
                const int ii = ti * TS + k, jj = tj * TS + l;
                if (ii <= jj && jj < M) { out[ii * M + jj] = acc[k][l]; out[jj * M + ii] = acc[k][l]; }
            }
    }
    if (tid < M) out[M * M + tid] = gacc;
    if (tid == 255) { out[M * M + M] = s_dd; out[M * M + M + 1] = s_r; out[M * M + M + 2] = (double)s_n; }
}

hipError_t launch_letkf_patch_gram(const LetkfPatchGramArgs& a, hipStream_t s) {
    if (a.M < 2 || a.M > LNS_ETKF_MAX_MEMBERS || a.h < 1 || a.w < 1 || (long)a.h * a.w > LNS_LETKF_MAX_DOMAINS) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(a.h * a.w), (unsigned)a.B, (unsigned)a.kk);
    if (a.M <= 32) {
        const size_t lds = (size_t)(2 * 64 * (16 * 2 + 2) + 3 * 64) * sizeof(double);
        hipLaunchKernelGGL(letkf_patch_gram_kernel<2>, grid, dim3(256), lds, s, a);
    } else {
        const size_t lds = (size_t)(2 * 64 * (16 * 4 + 2) + 3 * 64) * sizeof(double);   // 69120 bytes
        hipLaunchKernelGGL(letkf_patch_gram_kernel<4>, grid, dim3(256), lds, s, a);
    }
    return hipGetLastError();
}

// The Gaspari-Cohn taper of include/lns.h at r >= 0: powers by repeated multiplication (r2 = r r, r3 = r2 r, r4 = r3 r,
// r5 = r4 r), the terms added from the left in the order written, nothing fused.
__device__ __forceinline__ double letkf_taper(double r) {
#pragma clang fp contract(off)
    if (r >= 2.0) return 0.0;
    const double r2 = r * r, r3 = r2 * r, r4 = r3 * r, r5 = r4 * r;
    if (r <= 1.0) return (((1.0 - (5.0 / 3.0) * r2) + (5.0 / 8.0) * r3) + 0.5 * r4) - 0.25 * r5;
    const double v = (((((4.0 - 5.0 * r) + (5.0 / 3.0) * r2) + (5.0 / 8.0) * r3) - 0.5 * r4) + (1.0 / 12.0) * r5) - 2.0 / (3.0 * r);
    return v > 0.0 ? v : 0.0;
}

// A block owns LNS_LETKF_DPB consecutive domains of one sample (their supports overlap, so every patch sum is read once for all
// of them), or, as the last block of a sample, the global sums.  LDS: the taper of each of its domains against every patch, and
// the ascending list of the patches with a positive weight in any of them (wave 0 compacts it by ballots).
#define LNS_LETKF_DPB 4
__global__ __launch_bounds__(256) void letkf_combine_kernel(LetkfCombineArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int M = a.M, MM = M * M, E = MM + M + 3, hw = a.h * a.w;
    double* wt = reinterpret_cast<double*>(smem);      // [LNS_LETKF_DPB][h * w] rho of the block's domains against every patch
    int* list = reinterpret_cast<int*>(wt + (size_t)LNS_LETKF_DPB * hw);   // [h * w] the patches some domain of the block weights
    int* cnt = list + hw;
    const int b = blockIdx.y, tid = threadIdx.x;
    const int nblk = (hw + LNS_LETKF_DPB - 1) / LNS_LETKF_DPB;
    const bool glob = (int)blockIdx.x == nblk;
    const int l0 = glob ? 0 : (int)blockIdx.x * LNS_LETKF_DPB;
    for (int k = tid; k < LNS_LETKF_DPB * hw; k += 256) {
        const int d = k / hw, t = k - d * hw, l = l0 + d;
        double rho = 0.0;
        if (glob) rho = d == 0 ? 1.0 : 0.0;
        else if (l < hw) {
            const int li = l / a.w, lj = l - li * a.w, ti = t / a.w, tj = t - ti * a.w;
            int dy = li > ti ? li - ti : ti - li, dx = lj > tj ? lj - tj : tj - lj;
            if (a.bc_y == 0 && a.h - dy < dy) dy = a.h - dy;      // periodic: min(dy, h - dy)
            if (a.bc_x == 0 && a.w - dx < dx) dx = a.w - dx;
            const double dist = sqrt((double)(dy * dy + dx * dx));
            rho = letkf_taper(dist / a.radius);
        }
        wt[k] = rho;
    }
    __syncthreads();
    if (tid < 64) {                                    // wave 0: lane = tid
        int base = 0;
        for (int t0 = 0; t0 < hw; t0 += 64) {
            const int t = t0 + tid;
            bool act = false;
            if (t < hw)
                for (int d = 0; d < LNS_LETKF_DPB; ++d) act = act || wt[d * hw + t] > 0.0;
            const unsigned long long m = __builtin_amdgcn_ballot_w64(act);
            if (act) list[base + __popcll(m & ((1ull << tid) - 1ull))] = t;
            base += __popcll(m);
        }
        if (tid == 0) *cnt = base;
    }
    __syncthreads();
    const int nl = *cnt;
    const double* src = a.part + (size_t)b * a.n * hw * E;
    const int e = (int)blockIdx.z * 256 + tid;         // one entry of (S, g) a thread; blockIdx.z walks the entries in chunks of 256
    if (e < MM + M) {
        int from = e;
        if (e < MM) { const int i = e / M, j = e - i * M; if (i > j) from = j * M + i; }
        double acc[LNS_LETKF_DPB];
#pragma unroll
        for (int d = 0; d < LNS_LETKF_DPB; ++d) acc[d] = 0.0;
        for (int i = 0; i < a.n; ++i)
            for (int k0 = 0; k0 < nl; k0 += 8) {       // eight independent loads ahead of the adds, which stay in ascending order
                double G[8];
                int tt[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    tt[u] = list[k0 + u < nl ? k0 + u : nl - 1];
                    G[u] = src[((size_t)i * hw + tt[u]) * E + from];
                }
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (k0 + u < nl) {
#pragma unroll
                        for (int d = 0; d < LNS_LETKF_DPB; ++d) {
                            const double rho = wt[d * hw + tt[u]];
                            if (rho > 0.0) acc[d] = acc[d] + rho * G[u];
                        }
                    }
            }
        if (glob) {
            if (e < MM) a.S_glob[(size_t)b * MM + e] = acc[0]; else a.g_glob[(size_t)b * M + (e - MM)] = acc[0];
        } else {
#pragma unroll
            for (int d = 0; d < LNS_LETKF_DPB; ++d)
                if (l0 + d < hw) {
                    if (e < MM) a.S_loc[((size_t)b * hw + l0 + d) * MM + e] = acc[d];
                    else a.g_loc[((size_t)b * hw + l0 + d) * M + (e - MM)] = acc[d];
                }
        }
    }
    if (glob && a.stat && blockIdx.z == 0)             // stat [B][n][3]: per step, the patches in ascending order
        for (int q = tid; q < a.n * 3; q += 256) {
            const int i = q / 3, k = q - i * 3;
            double acc = 0.0;
            for (int t = 0; t < hw; ++t) acc = acc + src[((size_t)i * hw + t) * E + MM + M + k];
            a.stat[((size_t)b * a.n + i) * 3 + k] = acc;
        }
}

hipError_t launch_letkf_combine(const LetkfCombineArgs& a, hipStream_t s) {
    if (a.M < 2 || a.M > LNS_ETKF_MAX_MEMBERS || a.n < 1 || a.h < 1 || a.w < 1 || (long)a.h * a.w > LNS_LETKF_MAX_DOMAINS ||
        !(a.radius > 0.0) || a.B < 1 || a.B > 65535)
        return hipErrorInvalidValue;
    const int hw = a.h * a.w, nblk = (hw + LNS_LETKF_DPB - 1) / LNS_LETKF_DPB;
    const size_t lds = (size_t)LNS_LETKF_DPB * hw * sizeof(double) + ((size_t)hw + 4) * sizeof(int);   // 147472 bytes at 4096 domains
    const unsigned nz = (unsigned)((a.M * a.M + a.M + 255) / 256);
    hipLaunchKernelGGL(letkf_combine_kernel, dim3((unsigned)nblk + 1, (unsigned)a.B, nz), dim3(256), lds, s, a);
    return hipGetLastError();
}

// z [B][M][c][hw] -> out [B][M][c][hw] (may be z) under X [B][hw][M][M]: the block of (l, b) walks the c channels in chunks of
// 64; a chunk's M x 64 values are in LDS before any of its outputs is written, and no other block touches pixel l of sample b.
__global__ __launch_bounds__(256) void letkf_update_kernel(LetkfUpdateArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int M = a.M, MM = M * M, l = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    double* Xs = reinterpret_cast<double*>(smem);      // [M][M]
    double* zb = Xs + MM;                              // [64] zbar of the chunk's channels
    float* zs = reinterpret_cast<float*>(zb + 64);     // [64][M] the chunk's values, channel-major
    const double* X = a.X + ((size_t)b * a.hw + l) * MM;
    for (int k = tid; k < MM; k += 256) Xs[k] = X[k];
    const long n = (long)a.c * a.hw;                   // elements of one member
    const float* zi = a.z + (long)b * M * n + l;
    float* zo = a.out + (long)b * M * n + l;
    for (int c0 = 0; c0 < a.c; c0 += 64) {
        const int cc = a.c - c0 < 64 ? a.c - c0 : 64;
        __syncthreads();                               // the last chunk's readers are done (and, the first time, Xs is complete)
        for (int w = tid; w < cc * M; w += 256) {
            const int k = w / cc, ch = w - k * cc;
            zs[ch * M + k] = zi[(long)k * n + (long)(c0 + ch) * a.hw];
        }
        __syncthreads();
        if (tid < cc) {
            double sum = 0.0;
            for (int k = 0; k < M; ++k) sum = sum + (double)zs[tid * M + k];
            zb[tid] = sum / (double)M;
        }
        __syncthreads();
        for (int w = tid; w < cc * M; w += 256) {
            const int ch = w / M, m = w - ch * M;
            const double zbar = zb[ch];
            double acc = 0.0;
            for (int k = 0; k < M; ++k) {
                const double Z = (double)zs[ch * M + k] - zbar;
                const double t = Z * Xs[k * M + m];
                acc = acc + t;
            }
            zo[(long)m * n + (long)(c0 + ch) * a.hw] = (float)(zbar + acc);
        }
    }
}

hipError_t launch_letkf_update(const LetkfUpdateArgs& a, hipStream_t s) {
    if (a.M < 2 || a.M > LNS_ETKF_MAX_MEMBERS || a.B < 1 || a.B > 65535 || a.c < 1 || a.hw < 1 || a.hw > LNS_LETKF_MAX_DOMAINS)
        return hipErrorInvalidValue;
    const size_t lds = ((size_t)a.M * a.M + 64) * sizeof(double) + (size_t)64 * a.M * sizeof(float);   // 49664 bytes at M = 64
    hipLaunchKernelGGL(letkf_update_kernel, dim3((unsigned)a.hw, (unsigned)a.B), dim3(256), lds, s, a);
    return hipGetLastError();
}

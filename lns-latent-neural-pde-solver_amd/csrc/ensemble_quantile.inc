// ---- ensemble quantiles and exceedance probabilities (lns_kernels.h EnsembleQuantileArgs; the statement: include/lns.h) ----
// Every output is per pixel, so the grid is (pixel tiles of 256, planes (j, b, c)): one pixel per thread, no reduction across
// pixels, no barrier, no atomics.  A pixel's M denormalised member values live in the thread's own LDS column
// col[m * 256 + tid] (lane-strided dwords: no bank conflict; nobody else touches the column) as the sort keys of the
// statement, key(x) = bits ^ (sign ? 0xFFFFFFFF : 0x80000000): an insertion sort while loading keeps the column ascending
// (about M * M / 4 moves), the order statistics are read back by index, the exceedance counts walk the column once per
// threshold.  M is a run-time value: there is no member array in registers.  Nothing is fused.
__device__ __forceinline__ unsigned quantile_key(float x) {
    const unsigned u = __float_as_uint(x);
    return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float quantile_value(unsigned k) {
    return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}

__global__ __launch_bounds__(256) void ensemble_quantile_kernel(EnsembleQuantileArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) char smem[];   // all dynamic (as ensemble_score_kernel): [M][256] keys
    const int tid = threadIdx.x;
    const int HW = a.H * a.W, M = a.M;
    const int i = blockIdx.x * 256 + tid;
    if (i >= HW) return;                               // (no barrier below)
    const int q = a.q0 + blockIdx.y;                   // (j * B + b) * C + c
    const int c = q % a.C, s = q / a.C, b = s % a.B, j = s / a.B;
    const long mstride = (long)a.C * HW;               // member to member inside frames [kk][B][M][C][HW]
    const float* f = a.frames + ((long)s * M * a.C + c) * HW + i;
    const auto [sd, mean, lo, hi, walls, clampv] = ChannelNorm(a.norm, c);
    bool zero = false;
    if (walls) { const int r = i / a.W, cx = i - r * a.W; zero = r == 0 || r == a.H - 1 || cx == 0 || cx == a.W - 1; }
    unsigned* col = reinterpret_cast<unsigned*>(smem) + tid;
    for (int m = 0; m < M; ++m) {
        float v = f[m * mstride];
        if (a.denorm) v = score_denorm(v, sd, mean, zero, clampv, lo, hi);
        const unsigned k = quantile_key(v);
        int n = m;
        for (; n > 0; --n) {
            const unsigned p = col[(n - 1) * 256];
            if (p <= k) break;
            col[n * 256] = p;
        }
        col[n * 256] = k;
    }
    const long plane = (long)b * a.o_T + a.o_t + j;    // (b, kept step) of the outputs
    for (int k = 0; k < a.n_q; ++k) {
        const int l = a.lo[k];
        const float fr = a.frac[k];
        float r = quantile_value(col[l * 256]);
        if (fr != 0.0f) {
            const float d = quantile_value(col[(l + 1) * 256]) - r;
            const float t = fr * d;
            r = r + t;
        }
        a.quant[((plane * a.n_q + k) * a.C + c) * HW + i] = r;
    }
    const float fm = (float)M;
    for (int k = 0; k < a.n_thr; ++k) {
        const float th = a.thr[k][c];
        int cnt = 0;
#pragma unroll 4
        for (int m = 0; m < M; ++m) cnt += quantile_value(col[m * 256]) > th ? 1 : 0;
        a.prob[((plane * a.n_thr + k) * a.C + c) * HW + i] = (float)cnt / fm;
    }
}

hipError_t launch_ensemble_quantile(const EnsembleQuantileArgs& a, hipStream_t s) {
    if (a.M < 1 || a.M > LNS_SCORE_MAX_MEMBERS || a.n_q < 0 || a.n_q > LNS_QUANTILE_MAX || a.n_thr < 0 || a.n_thr > LNS_QUANTILE_MAX)
        return hipErrorInvalidValue;
    for (int k = 0; k < a.n_q; ++k)
        if (a.lo[k] < 0 || a.lo[k] >= a.M || (a.lo[k] == a.M - 1 && a.frac[k] != 0.0f)) return hipErrorInvalidValue;
    const long planes = (long)a.kk * a.B * a.C;
    const unsigned tiles = (unsigned)(((long)a.H * a.W + 255) / 256);
    EnsembleQuantileArgs b = a;
    for (long q0 = 0; q0 < planes; q0 += 65535) {      // (the y extent of a grid ends at 65535)
        b.q0 = (int)q0;
        const unsigned ny = (unsigned)(planes - q0 < 65535 ? planes - q0 : 65535);
        hipLaunchKernelGGL(ensemble_quantile_kernel, dim3(tiles, ny), dim3(256), (size_t)a.M * 1024, s, b);
    }
    return hipGetLastError();
}

// ---- ensemble exceedance contingency tables (lns_kernels.h EnsembleExceedArgs; the statement: include/lns.h) ----
// The grid is the quantile kernel's: (pixel tiles of 256, planes (j, b, c)), one pixel per thread.  A thread reads its truth
// once and its M members in ascending order (consecutive lanes, consecutive pixels: every member read is coalesced) and
// keeps the eight counts n_k = #{m : v_m > thr[k][c]} in registers: no member column, no sort.  The block's table
// tab[k][o][n] lives in LDS ([n_thr][2][M + 1] int32, at most 8256 bytes, dynamic): zeroed, filled with one integer LDS
// atomic per (pixel, threshold), and after the barrier added to the plane's table with one global integer atomic per
// non-zero bin.  Integer adds commute and never round, so the table is the same bits whatever the block order, the
// grouping or the streams; the caller zeroes `table` ahead of the first launch.
__global__ __launch_bounds__(256) void ensemble_exceed_kernel(EnsembleExceedArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int* tab = reinterpret_cast<int*>(smem);
    const int tid = threadIdx.x;
    const int HW = a.H * a.W, M = a.M, M1 = a.M + 1;
    const int nbins = a.n_thr * 2 * M1;
    const int i = blockIdx.x * 256 + tid;
    const int q = a.q0 + blockIdx.y;                   // (j * B + b) * C + c
    const int c = q % a.C, s = q / a.C, b = s % a.B, j = s / a.B;
    for (int k = tid; k < nbins; k += 256) tab[k] = 0;
    __syncthreads();
    if (i < HW) {
        const long mstride = (long)a.C * HW;           // member to member inside frames [kk][B][M][C][HW]
        const float* f = a.frames + ((long)s * M * a.C + c) * HW + i;
        const float* g = a.y + (((long)b * a.y_T + a.y_t + j) * a.C + c) * HW + i;
        const auto [sd, mean, lo, hi, walls, clampv] = ChannelNorm(a.norm, c);
        bool zero = false;
        if (walls) { const int r = i / a.W, cx = i - r * a.W; zero = r == 0 || r == a.H - 1 || cx == 0 || cx == a.W - 1; }
        float th[LNS_EXCEED_MAX];
        int cnt[LNS_EXCEED_MAX];
#pragma unroll
        for (int k = 0; k < LNS_EXCEED_MAX; ++k) { th[k] = a.thr[k][c]; cnt[k] = 0; }   // (rows from n_thr on: 0, counted, never used)
        float qv = *g;
        if (a.denorm) qv = score_denorm(qv, sd, mean, zero, clampv, lo, hi);
#pragma unroll 4
        for (int m = 0; m < M; ++m) {
            float v = f[m * mstride];
            if (a.denorm) v = score_denorm(v, sd, mean, zero, clampv, lo, hi);
#pragma unroll
            for (int k = 0; k < LNS_EXCEED_MAX; ++k) cnt[k] += v > th[k] ? 1 : 0;
        }
#pragma unroll
        for (int k = 0; k < LNS_EXCEED_MAX; ++k)
            if (k < a.n_thr) atomicAdd(&tab[(k * 2 + (qv > th[k] ? 1 : 0)) * M1 + cnt[k]], 1);
    }
    __syncthreads();
    // tab[k][o][n] -> table[b][o_t + j][k][c][o][n] of table [B][o_T][n_thr][C][2][M + 1]
    const long plane = (long)b * a.o_T + a.o_t + j;
    for (int k = tid; k < nbins; k += 256) {
        const int v = tab[k];
        if (v == 0) continue;
        const int kt = k / (2 * M1), r = k - kt * 2 * M1;
        atomicAdd(a.table + ((plane * a.n_thr + kt) * a.C + c) * (2 * M1) + r, v);
    }
}

hipError_t launch_ensemble_exceed(const EnsembleExceedArgs& a, hipStream_t s) {
    if (a.M < 1 || a.M > LNS_SCORE_MAX_MEMBERS || a.n_thr < 1 || a.n_thr > LNS_EXCEED_MAX || a.C < 1 || a.C > LNS_METRIC_MAX_CH)
        return hipErrorInvalidValue;
    const long planes = (long)a.kk * a.B * a.C;
    const unsigned tiles = (unsigned)(((long)a.H * a.W + 255) / 256);
    const size_t lds = (size_t)a.n_thr * 2 * (a.M + 1) * sizeof(int);
    EnsembleExceedArgs b = a;
    for (long q0 = 0; q0 < planes; q0 += 65535) {      // (the y extent of a grid ends at 65535)
        b.q0 = (int)q0;
        const unsigned ny = (unsigned)(planes - q0 < 65535 ? planes - q0 : 65535);
        hipLaunchKernelGGL(ensemble_exceed_kernel, dim3(tiles, ny), dim3(256), lds, s, b);
    }
    return hipGetLastError();
}

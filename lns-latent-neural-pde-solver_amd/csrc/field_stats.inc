// ---- per-plane field statistics (lns_kernels.h FieldStatsArgs; the statement: include/lns.h "field statistics") ------
// One block of four waves owns one plane (b, step, c) and writes its LNS_FIELD_STATS floats and its 2 x (nbins + 2) counts
// itself.  The plane is walked three times (sums and extrema; centred sums; the two difference grids); every walk re-reads
// the two planes from global memory and denormalises on the way: a plane pair is at most 147 KB, which the second and
// third walk find in L2, and the block keeps no more LDS than its reduction slots and its counts (2.2 KB, static).
// (Staging the denormalised planes in LDS would give the same bits -- D_c is a function of the pixel -- but needs this
// path anyway for planes above 160 KB; DESIGN.md section 4.)  Every sum follows the order of the metric kernels: a
// thread's terms in ascending order from 0, wave_sum, then (w0 + w1) + (w2 + w3).  Nothing is fused.
#define LNS_FS_MAX_BINS 256

struct FsDenorm : ChannelNorm {
    int H, W;
    __device__ __forceinline__ FsDenorm(const FieldStatsArgs& a, int c) : ChannelNorm(a.norm, c), H(a.H), W(a.W) {}
    // pixel i = r * W + cx of a normalised plane p
    __device__ __forceinline__ float at(const float* p, int i, int r, int cx) const {
        const bool zero = walls && (r == 0 || r == H - 1 || cx == 0 || cx == W - 1);
        return score_denorm(p[i], sd, mean, zero, clampv, lo, hi);
    }
};

// row / column of a thread's terms tid, tid + 256, ... on a grid of width Wd, without a division per term
struct FsWalk {
    int r, cx, dq, dr, Wd;
    __device__ __forceinline__ FsWalk(int tid, int width) : r(tid / width), cx(tid % width), dq(256 / width), dr(256 % width), Wd(width) {}
    __device__ __forceinline__ void next() {
        cx += dr; r += dq;
        if (cx >= Wd) { cx -= Wd; ++r; }
    }
};

// k thread sums -> the k plane sums in every thread; red: k * 4 floats of LDS (a barrier on entry protects its last readers)
template <int K>
__device__ __forceinline__ void fs_block_sums(float (&v)[K], float* red) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const float w = wave_sum(v[k]);
        if ((tid & 63) == 0) red[k * 4 + (tid >> 6)] = w;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = (red[k * 4] + red[k * 4 + 1]) + (red[k * 4 + 2] + red[k * 4 + 3]);
}

__device__ __forceinline__ float fs_wave_min(float v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = fminf(v, __shfl_xor(v, m, 64));
    return v;
}
__device__ __forceinline__ float fs_wave_max(float v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
    return v;
}

// bin of a value (include/lns.h): 0 below lo, nbins + 1 from hi on, -1 for a NaN
__device__ __forceinline__ int fs_bin(float v, float lo, float hi, float scale, int nbins) {
#pragma clang fp contract(off)
    if (v < lo) return 0;
    if (v >= hi) return nbins + 1;
    if (!(v == v)) return -1;
    const float t = v - lo;
    const float u = t * scale;
    return 1 + min(nbins - 1, (int)u);
}

// f, g: the normalised forecast / truth plane; stats: LNS_FIELD_STATS floats; hist (nullable): 2 x (nbins + 2) counts
__device__ __forceinline__ void field_stats_plane(const float* f, const float* g, float* stats, int* hist, const FsDenorm& D,
                                                  float eps, int nbins, float hlo, float hhi, float hscale, float* red, int* cnt) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    const int H = D.H, W = D.W, HW = H * W;
    const float N = (float)HW;
    if (hist)
        for (int k = tid; k < 2 * (nbins + 2); k += 256) cnt[k] = 0;
    __syncthreads();                                           // the counts are zero before the first atomic
    // pass 1: SP, SQ, PP, QQ, PQ, the extrema and the counts
    float s1[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    float mnP = INFINITY, mxP = -INFINITY, mnQ = INFINITY, mxQ = -INFINITY;
    FsWalk w1(tid, W);
#pragma unroll 4
    for (int i = tid; i < HW; i += 256, w1.next()) {
        const int r = w1.r, cx = w1.cx;
        const float p = D.at(f, i, r, cx), q = D.at(g, i, r, cx);
        const float pp = p * p, qq = q * q, pq = p * q;
        s1[0] = s1[0] + p; s1[1] = s1[1] + q; s1[2] = s1[2] + pp; s1[3] = s1[3] + qq; s1[4] = s1[4] + pq;
        mnP = fminf(mnP, p); mxP = fmaxf(mxP, p); mnQ = fminf(mnQ, q); mxQ = fmaxf(mxQ, q);
        if (hist) {
            const int bp = fs_bin(p, hlo, hhi, hscale, nbins), bq = fs_bin(q, hlo, hhi, hscale, nbins);
            if (bp >= 0) atomicAdd(&cnt[bp], 1);
            if (bq >= 0) atomicAdd(&cnt[nbins + 2 + bq], 1);
        }
    }
    fs_block_sums(s1, red);
    mnP = fs_wave_min(mnP); mxP = fs_wave_max(mxP); mnQ = fs_wave_min(mnQ); mxQ = fs_wave_max(mxQ);
    float* ext = red + 20;                                     // [4 kinds][4 waves], read by thread 0 after the next barrier
    if ((tid & 63) == 0) { const int w = tid >> 6; ext[w] = mnP; ext[4 + w] = mxP; ext[8 + w] = mnQ; ext[12 + w] = mxQ; }
    const float mP = s1[0] / N, mQ = s1[1] / N;
    // pass 2: the centred sums
    float s2[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    FsWalk w2(tid, W);
#pragma unroll 4
    for (int i = tid; i < HW; i += 256, w2.next()) {
        const int r = w2.r, cx = w2.cx;
        const float a = D.at(f, i, r, cx) - mP, b = D.at(g, i, r, cx) - mQ;
        const float aa = a * a, bb = b * b, ab = a * b;
        s2[0] = s2[0] + a; s2[1] = s2[1] + b; s2[2] = s2[2] + aa; s2[3] = s2[3] + bb; s2[4] = s2[4] + ab;
    }
    fs_block_sums(s2, red);
    // the difference grids: (H - 2) x W, term i pairs pixel i with pixel i + 2 W; H x (W - 2), term (r, cx) pairs cx with cx + 2
    float s3[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (H >= 3 && W >= 3) {
        const int ny = (H - 2) * W;
        FsWalk wy(tid, W);
#pragma unroll 4
        for (int i = tid; i < ny; i += 256, wy.next()) {
            const int r = wy.r, cx = wy.cx;
            const float gp = D.at(f, i + 2 * W, r + 2, cx) - D.at(f, i, r, cx);
            const float gq = D.at(g, i + 2 * W, r + 2, cx) - D.at(g, i, r, cx);
            const float d = gp - gq;
            const float dd = d * d, gg = gq * gq;
            s3[0] = s3[0] + dd; s3[1] = s3[1] + gg;
        }
        const int Wx = W - 2, nx = H * Wx;
        FsWalk wx(tid, Wx);
#pragma unroll 4
        for (int i = tid; i < nx; i += 256, wx.next()) {
            const int r = wx.r, cx = wx.cx, j = r * W + cx;
            const float gp = D.at(f, j + 2, r, cx + 2) - D.at(f, j, r, cx);
            const float gq = D.at(g, j + 2, r, cx + 2) - D.at(g, j, r, cx);
            const float d = gp - gq;
            const float dd = d * d, gg = gq * gq;
            s3[2] = s3[2] + dd; s3[3] = s3[3] + gg;
        }
    }
    fs_block_sums(s3, red);                                    // its barriers also order ext and the counts before the reads below
    if (tid == 0) {
        float vP, vQ, cov;
        { const float c = s2[0] * s2[0]; const float k = c / N; const float n = s2[2] - k; vP = fmaxf(n / N, 0.0f); }
        { const float c = s2[1] * s2[1]; const float k = c / N; const float n = s2[3] - k; vQ = fmaxf(n / N, 0.0f); }
        { const float c = s2[0] * s2[1]; const float k = c / N; const float n = s2[4] - k; cov = n / N; }
        const float den = sqrtf(vP) * sqrtf(vQ);
        const float nP = sqrtf(s1[2]) + eps, nQ = sqrtf(s1[3]) + eps;
        const float nn = nP * nQ;
        stats[0] = mP; stats[1] = mQ; stats[2] = vP; stats[3] = vQ;
        stats[4] = den == 0.0f ? 0.0f : cov / den;
        stats[5] = s1[4] / nn;
        stats[6] = sqrtf(s3[0] / (s3[1] < eps ? eps : s3[1]));
        stats[7] = sqrtf(s3[2] / (s3[3] < eps ? eps : s3[3]));
        stats[8] = fminf(fminf(ext[0], ext[1]), fminf(ext[2], ext[3]));
        stats[9] = fmaxf(fmaxf(ext[4], ext[5]), fmaxf(ext[6], ext[7]));
        stats[10] = fminf(fminf(ext[8], ext[9]), fminf(ext[10], ext[11]));
        stats[11] = fmaxf(fmaxf(ext[12], ext[13]), fmaxf(ext[14], ext[15]));
    }
    if (hist)
        for (int k = tid; k < 2 * (nbins + 2); k += 256) hist[k] = cnt[k];
}

__device__ __forceinline__ void field_stats_block(const FieldStatsArgs& a, const float* f, const float* g, long oplane, int c) {
    __shared__ float red[36];                                  // 5 x 4 wave sums, 4 x 4 wave extrema
    __shared__ int cnt[2 * (LNS_FS_MAX_BINS + 2)];
    const FsDenorm D(a, c);
    const int hc = a.hist ? c : 0;                             // (histograms: C <= 8, checked on the host)
    field_stats_plane(f, g, a.stats + oplane * LNS_FIELD_STATS_N, a.hist ? a.hist + oplane * 2 * (a.nbins + 2) : nullptr, D,
                      a.eps, a.nbins, a.hlo[hc], a.hhi[hc], a.hscale[hc], red, cnt);
}

// frames [kk][B][C][H*W] (a decode stream's frame buffer): block q = (i * B + b) * C + c takes step j = sel[i] of the group
__global__ __launch_bounds__(256) void field_stats_group_kernel(FieldStatsArgs a) {
    const int q = blockIdx.x;
    const int c = q % a.C, s = q / a.C, b = s % a.B, i = s / a.B;
    const int j = a.sel[i];
    const long HW = (long)a.H * a.W;
    const float* f = a.frames + (((long)j * a.B + b) * a.C + c) * HW;
    const float* g = a.y + (((long)b * a.y_T + a.y_t + j) * a.C + c) * HW;
    field_stats_block(a, f, g, ((long)b * a.o_T + a.o_t + i) * a.C + c, c);
}

// stored fields yhat / y [B][T][C][H*W]: block = plane
__global__ __launch_bounds__(256) void field_stats_stored_kernel(FieldStatsArgs a) {
    const long p = blockIdx.x;
    const long HW = (long)a.H * a.W;
    field_stats_block(a, a.frames + p * HW, a.y + p * HW, p, (int)(p % a.C));
}

static bool field_stats_args_ok(const FieldStatsArgs& a) {
    if (!a.frames || !a.y || !a.stats || a.B < 1 || a.C < 1 || a.H < 1 || a.W < 1 || (long)a.H * a.W > (1L << 30)) return false;
    if (a.norm.per_channel && a.C > LNS_METRIC_MAX_CH) return false;
    if (a.hist && (a.nbins < 1 || a.nbins > LNS_FS_MAX_BINS || a.C > LNS_METRIC_MAX_CH)) return false;
    return true;
}

hipError_t launch_field_stats_group(const FieldStatsArgs& a, hipStream_t s) {
    if (!field_stats_args_ok(a) || a.n < 1 || a.n > 8) return hipErrorInvalidValue;
    hipLaunchKernelGGL(field_stats_group_kernel, dim3((unsigned)((long)a.n * a.B * a.C)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_field_stats_stored(const FieldStatsArgs& a, hipStream_t s) {
    if (!field_stats_args_ok(a) || a.n < 1 || (long)a.n * a.B * a.C > 0x7fffffffL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(field_stats_stored_kernel, dim3((unsigned)((long)a.n * a.B * a.C)), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ---- flow diagnostics across the two velocity channels (lns_kernels.h FlowStatsArgs; the statement: include/lns.h "flow diagnostics") ------
// Statistics: one block of four waves owns one frame (b, step) and writes its LNS_FLOW_STATS_N floats and its 2 x (nbins + 2)
// counts itself.  The frame is walked once; every pixel reads its own value and its two neighbours along each axis of both
// velocity planes of forecast and truth from global memory (20 neighbour loads, which the planes' 64 KB each keep in L2) and
// denormalises on the way: the wall-zero rule of D_c belongs to the position a value is read at, so a neighbour on the wall is
// zero for the stencil as it is for the field.  (Staging rows in LDS would give the same bits but needs this path anyway for
// planes that do not fit; DESIGN.md section 4.)  Every sum follows the order of the metric kernels (fs_block_sums,
// field_stats.inc).  Vorticity frames: pointwise, one thread per pixel, the same pixel function.  Nothing is fused.
struct FlDenorm : ChannelNorm {
    int H, W;
    __device__ __forceinline__ FlDenorm(const ScoreNorm& n, int c, int H_, int W_) : ChannelNorm(n, c), H(H_), W(W_) {}
    // pixel (r, cx) of a normalised plane p
    __device__ __forceinline__ float at(const float* p, int r, int cx) const {
        const bool zero = walls && (r == 0 || r == H - 1 || cx == 0 || cx == W - 1);
        return score_denorm(p[r * W + cx], sd, mean, zero, clampv, lo, hi);
    }
};

struct FlowGeom {
    int H, W;
    bool wall_y, wall_x;
    float rcy, rey, rcx, rex;
    __device__ __forceinline__ explicit FlowGeom(const FlowStatsArgs& a)
        : H(a.H), W(a.W), wall_y(a.bc_y != 0), wall_x(a.bc_x != 0), rcy(a.rcy), rey(a.rey), rcx(a.rcx), rex(a.rex) {}
};

// The derivative at index i of an axis of length n >= 2 is (f[hi] - f[lo]) * s: one-sided at the two ends of a wall axis,
// central elsewhere, wrapped on a periodic axis.  0 <= lo, hi < n for every 0 <= i < n.
__device__ __forceinline__ void flow_stencil(int i, int n, bool wall, float rc, float re, int& lo, int& hi, float& s) {
    if (wall) {
        lo = max(i - 1, 0); hi = min(i + 1, n - 1);
        s = (i == 0 || i == n - 1) ? re : rc;
    } else {
        lo = i == 0 ? n - 1 : i - 1; hi = i == n - 1 ? 0 : i + 1;
        s = rc;
    }
}

struct FlowPixel { float U, V, w, dv; };

// pixel (r, cx) of the normalised velocity planes pu, pv: U, V, vorticity and divergence.  The one pixel function of the
// statistics and of the vorticity frames.
__device__ __forceinline__ FlowPixel flow_pixel(const float* pu, const float* pv, const FlDenorm& Du, const FlDenorm& Dv,
                                                const FlowGeom& G, int r, int cx) {
#pragma clang fp contract(off)
    FlowPixel o;
    o.U = Du.at(pu, r, cx); o.V = Dv.at(pv, r, cx);
    float dxU = 0.0f, dxV = 0.0f, dyU = 0.0f, dyV = 0.0f;
    if (G.W > 1) {
        int lo, hi; float s;
        flow_stencil(cx, G.W, G.wall_x, G.rcx, G.rex, lo, hi, s);
        const float du = Du.at(pu, r, hi) - Du.at(pu, r, lo);
        const float dv = Dv.at(pv, r, hi) - Dv.at(pv, r, lo);
        dxU = du * s; dxV = dv * s;
    }
    if (G.H > 1) {
        int lo, hi; float s;
        flow_stencil(r, G.H, G.wall_y, G.rcy, G.rey, lo, hi, s);
        const float du = Du.at(pu, hi, cx) - Du.at(pu, lo, cx);
        const float dv = Dv.at(pv, hi, cx) - Dv.at(pv, lo, cx);
        dyU = du * s; dyV = dv * s;
    }
    o.w = dxV - dyU;
    o.dv = dxU + dyV;
    return o;
}

// fu, fv / gu, gv: the normalised velocity planes of forecast / truth; stats: LNS_FLOW_STATS_N floats; hist (nullable):
// 2 x (nbins + 2) counts of the vorticity; red: 48 floats, cnt: 2 x (LNS_FS_MAX_BINS + 2) ints of LDS
__device__ __forceinline__ void flow_stats_plane(const float* fu, const float* fv, const float* gu, const float* gv, float* stats,
                                                 int* hist, const FlDenorm& Du, const FlDenorm& Dv, const FlowGeom& G, float eps,
                                                 int nbins, float hlo, float hhi, float hscale, float* red, int* cnt) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    const int HW = G.H * G.W;
    const float N = (float)HW;
    if (hist)
        for (int k = tid; k < 2 * (nbins + 2); k += 256) cnt[k] = 0;
    __syncthreads();                                           // the counts are zero before the first atomic
    // KP, KQ, WP, WQ, DP, DQ, WE, WX, VE
    float s[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    float mwP = 0.0f, mwQ = 0.0f, mdP = 0.0f;
    FsWalk wk(tid, G.W);
    for (int i = tid; i < HW; i += 256, wk.next()) {
        const FlowPixel p = flow_pixel(fu, fv, Du, Dv, G, wk.r, wk.cx);
        const FlowPixel q = flow_pixel(gu, gv, Du, Dv, G, wk.r, wk.cx);
        { const float uu = p.U * p.U, vv = p.V * p.V; const float k = uu + vv; s[0] = s[0] + k; }
        { const float uu = q.U * q.U, vv = q.V * q.V; const float k = uu + vv; s[1] = s[1] + k; }
        { const float ww = p.w * p.w; s[2] = s[2] + ww; }
        { const float ww = q.w * q.w; s[3] = s[3] + ww; }
        { const float dd = p.dv * p.dv; s[4] = s[4] + dd; }
        { const float dd = q.dv * q.dv; s[5] = s[5] + dd; }
        { const float e = p.w - q.w; const float ee = e * e; s[6] = s[6] + ee; }
        { const float x = p.w * q.w; s[7] = s[7] + x; }
        { const float a = p.U - q.U, b = p.V - q.V; const float aa = a * a, bb = b * b; const float v = aa + bb; s[8] = s[8] + v; }
        mwP = fmaxf(mwP, fabsf(p.w)); mwQ = fmaxf(mwQ, fabsf(q.w)); mdP = fmaxf(mdP, fabsf(p.dv));
        if (hist) {
            const int bp = fs_bin(p.w, hlo, hhi, hscale, nbins), bq = fs_bin(q.w, hlo, hhi, hscale, nbins);
            if (bp >= 0) atomicAdd(&cnt[bp], 1);
            if (bq >= 0) atomicAdd(&cnt[nbins + 2 + bq], 1);
        }
    }
    mwP = fs_wave_max(mwP); mwQ = fs_wave_max(mwQ); mdP = fs_wave_max(mdP);
    float* ext = red + 36;                                     // [3 kinds][4 waves]; fs_block_sums uses red[0 .. 36)
    if ((tid & 63) == 0) { const int w = tid >> 6; ext[w] = mwP; ext[4 + w] = mwQ; ext[8 + w] = mdP; }
    fs_block_sums(s, red);                                     // its barriers also order ext and the counts before the reads below
    if (tid == 0) {
        const float KP = s[0], KQ = s[1], WP = s[2], WQ = s[3], DP = s[4], DQ = s[5], WE = s[6], WX = s[7], VE = s[8];
        { const float h = 0.5f * KP; stats[0] = h / N; }
        { const float h = 0.5f * KQ; stats[1] = h / N; }
        { const float h = 0.5f * WP; stats[2] = h / N; }
        { const float h = 0.5f * WQ; stats[3] = h / N; }
        { const float m = DP / N; stats[4] = sqrtf(m); }
        { const float m = DQ / N; stats[5] = sqrtf(m); }
        { const float m = WE / (WQ < eps ? eps : WQ); stats[6] = sqrtf(m); }
        { const float nP = sqrtf(WP) + eps, nQ = sqrtf(WQ) + eps; const float nn = nP * nQ; stats[7] = WX / nn; }
        { const float m = VE / (KQ < eps ? eps : KQ); stats[8] = sqrtf(m); }
        stats[9] = fmaxf(fmaxf(ext[0], ext[1]), fmaxf(ext[2], ext[3]));
        stats[10] = fmaxf(fmaxf(ext[4], ext[5]), fmaxf(ext[6], ext[7]));
        stats[11] = fmaxf(fmaxf(ext[8], ext[9]), fmaxf(ext[10], ext[11]));
    }
    if (hist)
        for (int k = tid; k < 2 * (nbins + 2); k += 256) hist[k] = cnt[k];
}

// f / g: the normalised forecast / truth frame [C][H*W]; oframe: the frame's index in the outputs
__device__ __forceinline__ void flow_stats_block(const FlowStatsArgs& a, const float* f, const float* g, long oframe) {
    __shared__ float red[48];                                  // 9 x 4 wave sums, 3 x 4 wave maxima
    __shared__ int cnt[2 * (LNS_FS_MAX_BINS + 2)];
    const long HW = (long)a.H * a.W;
    const FlDenorm Du(a.norm, a.cu, a.H, a.W), Dv(a.norm, a.cv, a.H, a.W);
    const FlowGeom G(a);
    flow_stats_plane(f + a.cu * HW, f + a.cv * HW, g + a.cu * HW, g + a.cv * HW, a.stats + oframe * LNS_FLOW_STATS_N,
                     a.hist ? a.hist + oframe * 2 * (a.nbins + 2) : nullptr, Du, Dv, G, a.eps, a.nbins, a.hlo, a.hhi, a.hscale, red, cnt);
}

// frames [kk][B][C][H*W] (a decode stream's frame buffer): block q = i * B + b takes step j = sel[i] of the group
__global__ __launch_bounds__(256) void flow_stats_group_kernel(FlowStatsArgs a) {
    const int q = blockIdx.x;
    const int b = q % a.B, i = q / a.B;
    const int j = a.sel[i];
    const long per = (long)a.C * a.H * a.W;
    flow_stats_block(a, a.frames + ((long)j * a.B + b) * per, a.y + ((long)b * a.y_T + a.y_t + j) * per, (long)b * a.o_T + a.o_t + i);
}

// stored fields yhat / y [B][n][C][H*W]: block = frame
__global__ __launch_bounds__(256) void flow_stats_stored_kernel(FlowStatsArgs a) {
    const long p = blockIdx.x;
    const long per = (long)a.C * a.H * a.W;
    flow_stats_block(a, a.frames + p * per, a.y + p * per, p);
}

// the vorticity of one frame f [C][H*W] into out [H*W]: blockIdx.y strides over the frame's tiles of 256 pixels
__device__ __forceinline__ void vorticity_frame(const FlowStatsArgs& a, const float* f, float* out) {
    const int HW = a.H * a.W;
    const FlDenorm Du(a.norm, a.cu, a.H, a.W), Dv(a.norm, a.cv, a.H, a.W);
    const FlowGeom G(a);
    const float* pu = f + (long)a.cu * HW;
    const float* pv = f + (long)a.cv * HW;
    for (long p0 = (long)blockIdx.y * 256; p0 < HW; p0 += (long)gridDim.y * 256) {
        const int p = (int)p0 + (int)threadIdx.x;
        if (p < HW) {
            const int r = p / a.W;
            out[p] = flow_pixel(pu, pv, Du, Dv, G, r, p - r * a.W).w;
        }
    }
}

// frames [kk][B][C][H*W]: blockIdx.x = i * B + b takes step j = sel[i] of the group into vort[b][o_t + i] of vort [B][o_T][H*W]
__global__ __launch_bounds__(256) void vorticity_group_kernel(FlowStatsArgs a) {
    const int q = blockIdx.x;
    const int b = q % a.B, i = q / a.B;
    const int j = a.sel[i];
    const long HW = (long)a.H * a.W;
    vorticity_frame(a, a.frames + ((long)j * a.B + b) * a.C * HW, a.vort + ((long)b * a.o_T + a.o_t + i) * HW);
}

// stored fields [B][n][C][H*W] -> vort [B][n][H*W]: blockIdx.x = frame
__global__ __launch_bounds__(256) void vorticity_stored_kernel(FlowStatsArgs a) {
    const long p = blockIdx.x;
    const long HW = (long)a.H * a.W;
    vorticity_frame(a, a.frames + p * a.C * HW, a.vort + p * HW);
}

// frames: the launch's number of frames, below 2^24 (256 threads each: the grid's x extent stays below 2^32 threads)
static bool flow_args_ok(const FlowStatsArgs& a, long frames) {
    if (!a.frames || a.B < 1 || a.C < 2 || a.H < 1 || a.W < 1 || (long)a.H * a.W > (1L << 30)) return false;
    if (a.cu < 0 || a.cu >= a.C || a.cv < 0 || a.cv >= a.C || a.cu == a.cv) return false;
    if (a.norm.per_channel && a.C > LNS_METRIC_MAX_CH) return false;
    if (a.hist && (a.nbins < 1 || a.nbins > LNS_FS_MAX_BINS)) return false;
    return frames >= 1 && frames < (1L << 24);
}

hipError_t launch_flow_stats_group(const FlowStatsArgs& a, hipStream_t s) {
    if (!flow_args_ok(a, (long)a.n * a.B) || !a.y || !a.stats || a.n > 8) return hipErrorInvalidValue;
    hipLaunchKernelGGL(flow_stats_group_kernel, dim3((unsigned)(a.n * a.B)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_flow_stats_stored(const FlowStatsArgs& a, hipStream_t s) {
    if (!flow_args_ok(a, (long)a.n * a.B) || !a.y || !a.stats) return hipErrorInvalidValue;
    hipLaunchKernelGGL(flow_stats_stored_kernel, dim3((unsigned)((long)a.n * a.B)), dim3(256), 0, s, a);
    return hipGetLastError();
}

static unsigned vorticity_tiles(const FlowStatsArgs& a) { return (unsigned)std::min<long>(((long)a.H * a.W + 255) / 256, 256); }

hipError_t launch_vorticity_group(const FlowStatsArgs& a, hipStream_t s) {
    if (!flow_args_ok(a, (long)a.n * a.B) || !a.vort || a.n > 8) return hipErrorInvalidValue;
    hipLaunchKernelGGL(vorticity_group_kernel, dim3((unsigned)(a.n * a.B), vorticity_tiles(a)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_vorticity_stored(const FlowStatsArgs& a, hipStream_t s) {
    if (!flow_args_ok(a, (long)a.n * a.B) || !a.vort) return hipErrorInvalidValue;
    hipLaunchKernelGGL(vorticity_stored_kernel, dim3((unsigned)((long)a.n * a.B), vorticity_tiles(a)), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ---- error attribution (lns_kernels.h AttribGroupArgs / LatentErrArgs; the statement: include/lns.h "error attribution") ----
// The rollout error of a plane split at the reconstruction r = D(E(y)) of the truth: a = D_c(yhat) - D_c(r) is what the
// propagator adds, b = D_c(r) - D_c(y) what the autoencoder leaves.  This kernel forms PP = sum a a, XX = sum a b and the
// denominator G = sum D_c(y)^2 of prop and cross; RR = sum b b over the metric's own G is the metric's pair for the
// reconstruction (metric_group_kernel on the second frame buffer), so the recon column is the metric's, bit for bit.
// One block of four waves per plane; a thread adds its terms tid, tid + 256, ... in ascending order from 0, one by one, then
// the wave sums and (w0 + w1) + (w2 + w3).  Nothing is fused, and no float4 grouping: three operands of three unrelated
// alignments would need eight orders.  G is summed in float64 (the products of fp32 values are exact there) in the same order
// and rounded to fp32 once: on a constant field -- 1e-12 x under a spec with a mean -- every thread of an fp32 sum rounds the
// same way, the metric's own G is 1.9e-7 off there, and cross, linear in 1 / g, would miss the project's rule by that alone.
__device__ __forceinline__ double attrib_wave_sum(double v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = v + __shfl_xor(v, m, 64);     // neighbours first: the balanced tree of wave_sum
    return v;
}

__global__ __launch_bounds__(256) void attrib_group_kernel(AttribGroupArgs a) {
#pragma clang fp contract(off)
    __shared__ float red[8];
    __shared__ double redg[4];
    const int q = blockIdx.x;                          // (j * B + b) * C + c
    const int c = q % a.C, s = q / a.C, b = s % a.B, j = s / a.B;
    const int HW = a.H * a.W;
    const float* f = a.frames + (long)q * HW;
    const float* r = a.recon + (long)q * HW;
    const float* g = a.y + (((long)b * a.y_T + a.y_t + j) * a.C + c) * HW;
    float* out3 = a.part + (((long)b * a.p_T + a.p_t + j) * a.C + c) * 3;
    const auto [sd, mean, lo, hi, walls, clampv] = ChannelNorm(a.norm, c);
    float pp = 0.0f, xx = 0.0f;
    double gg = 0.0;
    if (a.norm.per_channel) {                          // walls and clamp on all three operands, then the differences
        FsWalk w(threadIdx.x, a.W);
        for (int i = threadIdx.x; i < HW; i += 256, w.next()) {
            const bool zero = walls && (w.r == 0 || w.r == a.H - 1 || w.cx == 0 || w.cx == a.W - 1);
            const float P = score_denorm(f[i], sd, mean, zero, clampv, lo, hi);
            const float R = score_denorm(r[i], sd, mean, zero, clampv, lo, hi);
            const float Q = score_denorm(g[i], sd, mean, zero, clampv, lo, hi);
            const float da = P - R, db = R - Q;
            const float pa = da * da, px = da * db;
            pp = pp + pa; xx = xx + px;
            gg = gg + (double)Q * (double)Q;
        }
    } else {                                           // as the metric forms its error: the difference, then the scale
        for (int i = threadIdx.x; i < HW; i += 256) {
            const float rv = r[i], yv = g[i];
            const float d0 = f[i] - rv, d1 = rv - yv;
            const float da = d0 * sd, db = d1 * sd;
            const float pa = da * da, px = da * db;
            const float Q = score_denorm(yv, sd, mean, false, false, lo, hi);
            pp = pp + pa; xx = xx + px;
            gg = gg + (double)Q * (double)Q;
        }
    }
    gg = attrib_wave_sum(gg);
    if ((threadIdx.x & 63) == 0) redg[threadIdx.x >> 6] = gg;
    metric_plane_store(pp, xx, red, out3);             // (its barrier publishes redg too)
    if (threadIdx.x == 0) out3[2] = (float)((redg[0] + redg[1]) + (redg[2] + redg[3]));
}

// One block per (j, b): the metric's per-plane body on a latent pair.  n4 is what metric_plane_kernel would choose for plane
// (b, t + j) of stored [B][T_total][zper] tensors on 16-byte-aligned bases (the plane's offset decides); the staged true latent
// is aligned by construction (zstride), the ring slot is read by float4 only where it is.
__global__ __launch_bounds__(256) void latent_err_group_kernel(LatentErrArgs a) {
    __shared__ float red[8];
    const int b = blockIdx.x % a.B, j = blockIdx.x / a.B;
    const float* z = a.z + ((long)j * a.B + b) * a.zper;
    const float* zt = a.ztrue + ((long)j * a.B + b) * a.zstride;
    const long plane = (long)b * a.T_total + a.t + j;
    const int n4 = ((plane * a.zper) & 3) == 0 ? a.zper / 4 : 0;
    float d2 = 0.0f, g2 = 0.0f;
    if ((reinterpret_cast<uintptr_t>(z) & 15) == 0) metric_plane_sums<true>(z, zt, a.zper, n4, a.mean, a.sd, d2, g2);
    else metric_plane_sums<false>(z, zt, a.zper, n4, a.mean, a.sd, d2, g2);
    metric_plane_store(d2, g2, red, a.part + plane * 2);
}

// (b, c) per thread, t ascending, fp32: the frame-wise columns and, from the running sums, the sequence-wise ones, over the
// kernel's own G (pp[..][2])
__global__ void attrib_finish_kernel(const float* pp, int B, int T, int C, float eps, float* prop_frame,
                                     float* prop_seq, float* cross_frame, float* cross_seq) {
#pragma clang fp contract(off)
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;      // (b, c)
    if (idx >= B * C) return;
    const int b = idx / C, c = idx - b * C;
    float sp = 0.0f, sx = 0.0f, sg = 0.0f;
    for (int t = 0; t < T; ++t) {
        const long p = ((long)b * T + t) * C + c;
        const float PP = pp[p * 3], XX = pp[p * 3 + 1], g2 = pp[p * 3 + 2];
        const float g = g2 < eps ? eps : g2;
        if (prop_frame) prop_frame[p] = sqrtf(PP / g);
        if (cross_frame) cross_frame[p] = (2.0f * XX) / g;
        sp = sp + PP; sx = sx + XX; sg = sg + g2;
    }
    const float g = sg < eps ? eps : sg;
    if (prop_seq) prop_seq[idx] = sqrtf(sp / g);
    if (cross_seq) cross_seq[idx] = (2.0f * sx) / g;
}

hipError_t launch_attrib_group(const AttribGroupArgs& a, hipStream_t s) {
    if (a.kk < 1 || a.B < 1 || a.C < 1 || a.H < 1 || a.W < 1 || (long)a.kk * a.B * a.C > 0x7fffffffL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(attrib_group_kernel, dim3((unsigned)((long)a.kk * a.B * a.C)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_latent_err_group(const LatentErrArgs& a, hipStream_t s) {
    if (a.kk < 1 || a.B < 1 || a.zper < 1 || a.zstride < a.zper || (a.zstride & 3) || (reinterpret_cast<uintptr_t>(a.ztrue) & 15))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(latent_err_group_kernel, dim3((unsigned)(a.kk * a.B)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_attrib_finish(const float* pp, int B, int T, int C, float eps, float* prop_frame,
                                float* prop_seq, float* cross_frame, float* cross_seq, hipStream_t s) {
    hipLaunchKernelGGL(attrib_finish_kernel, dim3((B * C + 63) / 64), dim3(64), 0, s, pp, B, T, C, eps, prop_frame, prop_seq,
                       cross_frame, cross_seq);
    return hipGetLastError();
}

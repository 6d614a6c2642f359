// ---- per-pixel time maps (lns_kernels.h TimeMapsArgs; the statement: include/lns.h "time maps") -----------------------
// A thread owns V consecutive pixels of one (b, c) plane set and is the only writer of their state: it reads the six
// float64 sums and the fp32 running maximum once, adds the selected steps in ascending order and writes them back once.
// Nothing is reduced across threads, so there is no LDS, no barrier and no atomic, and the bits depend on the order of the
// steps alone.  The state is planar -- [6][N] doubles, then [N] floats, N = B * C * H * W -- so that a wave's loads of one
// sum are contiguous.  V = 4 (one 16-byte load per frame, two per sum) when H * W is a multiple of 4 and every pointer is
// 16-byte aligned, else V = 1.  Every float64 operation is rounded on its own (fp contract off).
#define LNS_TM_SUMS 6

template <int V>
__device__ __forceinline__ void tm_load(const float* p, float (&v)[V]) {
    if constexpr (V == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
        v[0] = *p;
    }
}
template <int V>
__device__ __forceinline__ void tm_store(float* p, const float (&v)[V]) {
    if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    else *p = v[0];
}
template <int V>
__device__ __forceinline__ void tm_load(const double* p, double (&v)[V]) {
    if constexpr (V == 4) {
        const double2 t0 = reinterpret_cast<const double2*>(p)[0], t1 = reinterpret_cast<const double2*>(p)[1];
        v[0] = t0.x; v[1] = t0.y; v[2] = t1.x; v[3] = t1.y;
    } else {
        v[0] = *p;
    }
}
template <int V>
__device__ __forceinline__ void tm_store(double* p, const double (&v)[V]) {
    if constexpr (V == 4) {
        reinterpret_cast<double2*>(p)[0] = make_double2(v[0], v[1]);
        reinterpret_cast<double2*>(p)[1] = make_double2(v[2], v[3]);
    } else {
        *p = v[0];
    }
}

// the denormalisation of channel c and which of the V pixels from `pix` (row-major in the plane) lie on a wall
template <int V>
struct TmDenorm : ChannelNorm {
    bool zero[V];
    __device__ __forceinline__ TmDenorm(const TimeMapsArgs& a, int c, int pix) : ChannelNorm(a.norm, c) {
#pragma unroll
        for (int u = 0; u < V; ++u) {
            const int r = (pix + u) / a.W, cx = (pix + u) % a.W;
            zero[u] = walls && (r == 0 || r == a.H - 1 || cx == 0 || cx == a.W - 1);
        }
    }
    __device__ __forceinline__ float at(float x, int u) const { return score_denorm(x, sd, mean, zero[u], clampv, lo, hi); }
};

// One thread's V pixels: f / g point at them in the forecast / truth frame of step index 0, consecutive step indices lie
// f_step / g_step floats apart, g0 points at them in the truth's first frame of the horizon; the n selected steps have the
// indices step(0) < step(1) < ...; idx: the pixels' index in the state planes of N entries each.
template <int V, class Step>
__device__ __forceinline__ void time_maps_accumulate(const TimeMapsArgs& a, const float* f, long f_step, const float* g, long g_step,
                                                     const float* g0, long idx, long N, int c, int pix, int n, Step step) {
#pragma clang fp contract(off)
    const TmDenorm<V> D(a, c, pix);
    double* sums = static_cast<double*>(a.state) + idx;
    float* mxp = reinterpret_cast<float*>(static_cast<double*>(a.state) + LNS_TM_SUMS * N) + idx;
    double S[LNS_TM_SUMS][V];
    float mx[V], k[V];
#pragma unroll
    for (int m = 0; m < LNS_TM_SUMS; ++m) tm_load<V>(sums + m * N, S[m]);
    tm_load<V>(mxp, mx);
    tm_load<V>(g0, k);
#pragma unroll
    for (int u = 0; u < V; ++u) k[u] = D.at(k[u], u);
    for (int i = 0; i < n; ++i) {
        const long j = step(i);
        float p[V], q[V];
        tm_load<V>(f + j * f_step, p);
        tm_load<V>(g + j * g_step, q);
#pragma unroll
        for (int u = 0; u < V; ++u) {
            const double P = (double)D.at(p[u], u), Q = (double)D.at(q[u], u), K = (double)k[u];
            const double da = P - K, db = Q - K, de = P - Q;
            const double aa = da * da, bb = db * db, ab = da * db, ee = de * de;
            S[0][u] = S[0][u] + da; S[1][u] = S[1][u] + db;
            S[2][u] = S[2][u] + aa; S[3][u] = S[3][u] + bb; S[4][u] = S[4][u] + ab; S[5][u] = S[5][u] + ee;
            mx[u] = fmaxf(mx[u], (float)fabs(de));
        }
    }
#pragma unroll
    for (int m = 0; m < LNS_TM_SUMS; ++m) tm_store<V>(sums + m * N, S[m]);
    tm_store<V>(mxp, mx);
}

// frames [kk][B][C][H*W] (a decode stream's frame buffer) against y [B][y_T][C][H*W], whose step y_t is the group's first:
// the steps sel[0 .. n) of the group.  Grid (chunks of 256 * V pixels of a trajectory's C * H * W, B).
template <int V>
__global__ __launch_bounds__(256) void time_maps_group_kernel(TimeMapsArgs a) {
    const long HW = (long)a.H * a.W, CHW = a.C * HW;
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * V;
    if (i >= CHW) return;
    const int b = blockIdx.y;
    const float* f = a.frames + b * CHW + i;
    const float* g0 = a.y + (long)b * a.y_T * CHW + i;
    time_maps_accumulate<V>(a, f, (long)a.B * CHW, g0 + a.y_t * CHW, CHW, g0, b * CHW + i, (long)a.B * CHW, (int)(i / HW), (int)(i % HW),
                            a.n, [&a](int s) { return (long)a.sel[s]; });
}

// stored fields frames / y [B][T][C][H*W]: the steps first, first + every, ... below T (n of them)
template <int V>
__global__ __launch_bounds__(256) void time_maps_stored_kernel(TimeMapsArgs a) {
    const long HW = (long)a.H * a.W, CHW = a.C * HW;
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * V;
    if (i >= CHW) return;
    const int b = blockIdx.y;
    const float* f = a.frames + (long)b * a.y_T * CHW + i;
    const float* g0 = a.y + (long)b * a.y_T * CHW + i;
    time_maps_accumulate<V>(a, f, CHW, g0, CHW, g0, b * CHW + i, (long)a.B * CHW, (int)(i / HW), (int)(i % HW), a.n,
                            [&a](int s) { return (long)a.first + (long)s * a.every; });
}

// state -> maps [B][C][LNS_TIME_MAPS_N][H*W]; count: the selected steps of the whole horizon (>= 1).  One pixel per thread.
__global__ __launch_bounds__(256) void time_maps_finish_kernel(TimeMapsArgs a) {
#pragma clang fp contract(off)
    const long HW = (long)a.H * a.W, CHW = a.C * HW, N = (long)a.B * CHW;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= CHW) return;
    const int b = blockIdx.y, c = (int)(i / HW), pix = (int)(i % HW);
    const long idx = b * CHW + i;
    const TmDenorm<1> D(a, c, pix);
    const double K = (double)D.at(a.y[(long)b * a.y_T * CHW + i], 0);
    const double* s = static_cast<const double*>(a.state) + idx;
    const double Sa = s[0], Sb = s[N], Saa = s[2 * N], Sbb = s[3 * N], Sab = s[4 * N], See = s[5 * N];
    const float mx = (reinterpret_cast<const float*>(static_cast<const double*>(a.state) + LNS_TM_SUMS * N))[idx];
    const double Nn = (double)a.count, d = (double)(a.count > 1 ? a.count - 1 : 1);
    const double ma = Sa / Nn, mb = Sb / Nn;
    double vP, vQ, cov;
    { const double t = Sa * Sa; const double k = t / Nn; const double n = Saa - k; const double v = n / d; vP = v > 0.0 ? v : 0.0; }
    { const double t = Sb * Sb; const double k = t / Nn; const double n = Sbb - k; const double v = n / d; vQ = v > 0.0 ? v : 0.0; }
    { const double t = Sa * Sb; const double k = t / Nn; const double n = Sab - k; cov = n / d; }
    float* o = a.maps + ((long)b * a.C + c) * LNS_TIME_MAPS_N * HW + pix;
    o[0] = (float)(K + ma); o[HW] = (float)(K + mb);
    o[2 * HW] = (float)vP; o[3 * HW] = (float)vQ; o[4 * HW] = (float)cov;
    o[5 * HW] = (float)(See / Nn); o[6 * HW] = mx;
}

static bool time_maps_args_ok(const TimeMapsArgs& a) {
    if (!a.y || !a.state || a.B < 1 || a.B > 65535 || a.C < 1 || a.H < 1 || a.W < 1 || (long)a.H * a.W > (1L << 30)) return false;
    if ((long)a.C * a.H * a.W > (1L << 38) || (reinterpret_cast<uintptr_t>(a.state) & 7)) return false;
    if (a.norm.per_channel && a.C > LNS_METRIC_MAX_CH) return false;
    return true;
}

// V = 4 needs every vector access on a 16-byte boundary: planes of a multiple of 4 pixels and aligned bases
static bool time_maps_vec4(const TimeMapsArgs& a) {
    const uintptr_t bits = reinterpret_cast<uintptr_t>(a.frames) | reinterpret_cast<uintptr_t>(a.y) | reinterpret_cast<uintptr_t>(a.state);
    return ((long)a.H * a.W) % 4 == 0 && (bits & 15) == 0;
}

hipError_t launch_time_maps_group(const TimeMapsArgs& a, hipStream_t s) {
    if (!time_maps_args_ok(a) || !a.frames || a.n < 1 || a.n > 8 || a.y_t < 0 || a.y_t + a.sel[a.n - 1] >= a.y_T) return hipErrorInvalidValue;
    const long CHW = (long)a.C * a.H * a.W;
    if (time_maps_vec4(a)) hipLaunchKernelGGL(time_maps_group_kernel<4>, dim3((unsigned)((CHW / 4 + 255) / 256), a.B), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(time_maps_group_kernel<1>, dim3((unsigned)((CHW + 255) / 256), a.B), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_time_maps_stored(const TimeMapsArgs& a, hipStream_t s) {
    if (!time_maps_args_ok(a) || !a.frames || a.n < 1 || a.first < 0 || a.every < 1 ||
        (long)a.first + (long)(a.n - 1) * a.every >= a.y_T) return hipErrorInvalidValue;
    const long CHW = (long)a.C * a.H * a.W;
    if (time_maps_vec4(a)) hipLaunchKernelGGL(time_maps_stored_kernel<4>, dim3((unsigned)((CHW / 4 + 255) / 256), a.B), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(time_maps_stored_kernel<1>, dim3((unsigned)((CHW + 255) / 256), a.B), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_time_maps_finish(const TimeMapsArgs& a, hipStream_t s) {
    if (!time_maps_args_ok(a) || !a.maps || a.count < 1 || a.y_T < 1) return hipErrorInvalidValue;
    const long CHW = (long)a.C * a.H * a.W;
    hipLaunchKernelGGL(time_maps_finish_kernel, dim3((unsigned)((CHW + 255) / 256), a.B), dim3(256), 0, s, a);
    return hipGetLastError();
}

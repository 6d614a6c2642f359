// ---------------------------------------------------------------------------------------------------------------------
// Batch-parallel weight gradient (included by lns_train_kernels.hip; engine option "train_wgrad" = 1).
//
// The same contraction as conv_wgrad_kernel,
//   dW[co][ci][ty][tx] = sum_b sum_{y,x} dY[b][co][y][x] * Xpad[b][ci][y + ty*dil][x + tx*dil],
// with K = (sample, 64-pixel chunk) cut into S slices of whole chunks in ascending (sample, chunk) order.  One block owns
// one (co tile, ci tile, slice): 256 threads = 4 waves = 64 (co) x 64 (ci), v_mfma_f32_32x32x2_f32, fp32 accumulate.  It
// writes its partial tile with plain stores to part[S][Cout][Cin][k*k]; wgrad_reduce_kernel sums the S partials of each
// weight element in ascending slice order (no floating-point atomics: the result is bit-reproducible for a shape).
//
// NINE (3x3): one block computes all nine taps from ONE staged dy chunk and ONE x patch -- the rows the chunk touches
// plus a halo of `dil` on every side, gathered through the whole-image rowmap / colmap (so circular / zero / half-periodic
// padding and the dilation keep coming from the maps) -- nine accumulator tiles per wave.  The patch is [position][ci] in
// LDS; a pixel's tap (ty, tx) is at position ppos[pixel] + ty*dil*PW + tx*dil.  Patches of more than WG_PATCH_MAX positions
// (very wide images) and 1x1 convolutions take the other form: the tap on the grid, x gathered per pixel.
// No per-element integer division: rows / columns of a chunk are stepped from the chunk's base (y0, x0), the staging
// loops decompose their index by shifts and nested loops.
// ---------------------------------------------------------------------------------------------------------------------
#define WG_PATCH_MAX 512                       // patch positions: 512 * 65 * 4 B + dy tile + tables = 149 KB of the 160 KB LDS

// upper bound of the image rows a 64-pixel chunk touches
static int wgrad_chunk_rows(int H, int W) {
    const int r = (WG_PX % W == 0) ? WG_PX / W : (W + WG_PX - 2) / W + 1;
    return r < H ? r : H;
}
static int wgrad_patch_positions(int H, int W, int k, int dil) {
    if (k != 3) return 0;
    const long n = (long)(wgrad_chunk_rows(H, W) + 2 * dil) * (W + 2 * dil);
    return n <= WG_PATCH_MAX ? (int)n : 0;     // 0: tap-on-grid form
}

// Slices of a launch: a function of the launch shape only.  About `target` blocks per launch, at most `smax` partials per
// element, every slice the same whole number of chunks (the last one may be shorter).  The two constants (WG_TARGET_BLOCKS,
// WG_MAX_SLICES in tools/wgrad_sweep.py's records) are the defaults of LNS_WGRAD_TARGET_BLOCKS / LNS_WGRAD_MAX_SLICES in
// lns_knobs.h, 512 and 128, from the sweep in profiles/wgrad_split_slices.txt: the step time is flat from one block per CU (256)
// up to four; two per CU is the middle of the plateau.  Read once per process, so that within a process S stays a function of
// the launch shape only.
int wgrad_split_slices(int B, int H, int W, int Cin, int Cout, int k) {
    (void)k;
    const long nchunk = ((long)H * W + WG_PX - 1) / WG_PX, NC = (long)B * nchunk;
    const long tiles = (long)((Cout + 63) / 64) * ((Cin + 63) / 64);
    const long target = knobs().wgrad_target_blocks, smax = knobs().wgrad_max_slices;
    long S = (target + tiles - 1) / tiles;
    if (S > smax) S = smax;
    if (S > NC) S = NC;
    if (S < 1) S = 1;
    const long cps = (NC + S - 1) / S;
    return (int)((NC + cps - 1) / cps);
}
size_t wgrad_split_scratch_floats(int B, int H, int W, int Cin, int Cout, int k) {
    return (size_t)wgrad_split_slices(B, H, W, Cin, Cout, k) * Cout * Cin * k * k;
}

template <bool NINE>
__global__ __launch_bounds__(256) void conv_wgrad_split_kernel(WgradArgs a) {
    extern __shared__ float wg_smem[];
    constexpr int NT = NINE ? 9 : 1;
    const int npos_max = NINE ? a.patch_pos : WG_PX;
    float* sdy = wg_smem;                                        // [pixel][co]
    float* sx = sdy + WG_PX * WG_LD;                             // NINE: [patch position][ci]; else [pixel][ci]
    int* psrc = reinterpret_cast<int*>(sx + npos_max * WG_LD);   // source offset sy * W + sx of a position / pixel, or -1
    int* ppos = psrc + npos_max;                                 // NINE: pixel -> patch position of its tap (0, 0)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int ci_tiles = (a.Cin + 63) >> 6;
    const int cot = blockIdx.y / ci_tiles, cit = blockIdx.y - cot * ci_tiles;      // once per block
    const int co0 = cot * 64, ci0 = cit * 64, slice = blockIdx.x;
    const int tap = NINE ? 0 : blockIdx.z;
    const int ty = tap / a.k, tx = tap - ty * a.k;
    const int HW = a.H * a.W, PW = a.W + 2 * a.dil;
    const int wm = wave >> 1, wn = wave & 1;                     // wave tile: co 32*wm.., ci 32*wn..
    const int l31 = lane & 31, kh = lane >> 5;
    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
    int toff[NT];                                                // LDS offset of tap t relative to tap (0, 0)
#pragma unroll
    for (int t = 0; t < NT; ++t) toff[t] = NINE ? ((t / 3) * a.dil * PW + (t % 3) * a.dil) * WG_LD : 0;

    const int NC = a.B * a.nchunk;
    const int c_begin = slice * a.cps, c_end = c_begin + a.cps < NC ? c_begin + a.cps : NC;
    int b = c_begin / a.nchunk, j = c_begin - b * a.nchunk;      // once per block; stepped below
    for (int c = c_begin; c < c_end; ++c) {
        const int p0 = j * WG_PX, npx = HW - p0 < WG_PX ? HW - p0 : WG_PX;
        const int y0 = p0 / a.W, x0 = p0 - y0 * a.W;             // the chunk's base: wave-uniform, once per chunk
        const float* dyb = a.dy + (long)b * a.Cout * HW;
        const float* xb = a.x + (long)b * a.x_bs;
        __syncthreads();                                         // the previous chunk's fragments have been read
        int npos = WG_PX;
        if (NINE) {
            const int y1 = (p0 + npx - 1) / a.W, PH = y1 - y0 + 1 + 2 * a.dil;
            npos = PH * PW;
            for (int pr = wave; pr < PH; pr += 4) {
                const int sy = a.rowmap[y0 + pr];
                for (int pc = lane; pc < PW; pc += 64) {
                    const int sc = a.colmap[pc];
                    psrc[pr * PW + pc] = (sy >= 0 && sc >= 0) ? sy * a.W + sc : -1;
                }
            }
            if (tid < WG_PX) {
                int col = x0 + tid, row = 0;
                while (col >= a.W) { col -= a.W; ++row; }
                ppos[tid] = tid < npx ? row * PW + col : 0;
            }
        } else if (tid < WG_PX) {
            int col = x0 + tid, row = y0;
            while (col >= a.W) { col -= a.W; ++row; }
            int off = -1;
            if (tid < npx) {
                const int sy = a.rowmap[row + ty * a.dil], sc = a.colmap[col + tx * a.dil];
                if (sy >= 0 && sc >= 0) off = sy * a.W + sc;
            }
            psrc[tid] = off;
        }
        __syncthreads();
        {   // dy chunk: thread -> pixel tid & 63, channels (tid >> 6) + 4 i; coalesced along pixels
            const int px = lane;
            const bool okp = px < npx;
#pragma unroll 8
            for (int i = 0; i < 16; ++i) {
                const int ch = wave + 4 * i;
                float vd = 0.0f;
                if (okp && co0 + ch < a.Cout) vd = dyb[(long)(co0 + ch) * HW + p0 + px];
                sdy[px * WG_LD + ch] = vd;
            }
        }
        for (int pos = lane; pos < npos; pos += 64) {            // x: patch positions (NINE) or pixels along the lanes
            const int off = psrc[pos];
#pragma unroll 8
            for (int i = 0; i < 16; ++i) {
                const int ch = wave + 4 * i;
                float vx = 0.0f;
                if (off >= 0 && ci0 + ch < a.Cin) vx = xb[(long)(ci0 + ch) * HW + off];
                sx[pos * WG_LD + ch] = vx;
            }
        }
        __syncthreads();
        const int ksteps = (npx + 1) >> 1;                       // pixel npx of an odd chunk is a zero row of sdy
        const float* pa = sdy + kh * WG_LD + wm * 32 + l31;
        const float* pb = sx + wn * 32 + l31;
        for (int ks = 0; ks < ksteps; ++ks) {
            const float av = pa[2 * ks * WG_LD];
            const float* q = pb + (NINE ? ppos[2 * ks + kh] : 2 * ks + kh) * WG_LD;
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, q[toff[t]], acc[t], 0, 0, 0);
        }
        if (++j == a.nchunk) { j = 0; ++b; }
    }
    // D[row = co][col = ci]: lane holds column l31, rows (r & 3) + 8 (r >> 2) + 4 kh
    const int kk = a.k * a.k;
    const int ci = ci0 + wn * 32 + l31;
    if (ci < a.Cin) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = co0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
            if (co < a.Cout) {
                float* d = a.part + (((long)slice * a.Cout + co) * a.Cin + ci) * kk + tap;
#pragma unroll
                for (int t = 0; t < NT; ++t) d[t] = acc[t][r];
            }
        }
    }
}

// dw[e] (+)= sum_s part[s][e], s ascending; one thread per weight element: coalesced over the [Cout][Cin][k*k] layout
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* part, float* dw, long n, int S, int accumulate) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = part[i];
    for (int sl = 1; sl < S; ++sl) s += part[(long)sl * n + i];
    dw[i] = accumulate ? dw[i] + s : s;
}

static size_t wgrad_split_lds(int npos) { return ((size_t)(WG_PX + npos) * WG_LD + npos + WG_PX) * 4; }

hipError_t init_train_kernels() {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(conv_wgrad_split_kernel<true>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)wgrad_split_lds(WG_PATCH_MAX));
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(conv_wgrad_split_kernel<false>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)wgrad_split_lds(WG_PX));
}

// a.part: S * Cout * Cin * k * k floats with S = a.S = wgrad_split_slices(...) of this shape
hipError_t launch_conv_wgrad_split(const WgradArgs& a0, hipStream_t s) {
    WgradArgs a = a0;
    if (a.S < 1 || !a.part || (a.k != 1 && a.k != 3)) return hipErrorInvalidValue;
    const long nchunk = ((long)a.H * a.W + WG_PX - 1) / WG_PX, NC = (long)a.B * nchunk;
    if (NC >= (1L << 31) || a.S > NC) return hipErrorInvalidValue;
    a.nchunk = (int)nchunk;
    a.cps = (int)((NC + a.S - 1) / a.S);
    if ((long)a.cps * (a.S - 1) >= NC) return hipErrorInvalidValue;                // every slice holds a chunk
    a.patch_pos = wgrad_patch_positions(a.H, a.W, a.k, a.dil);
    const int tiles = ((a.Cout + 63) / 64) * ((a.Cin + 63) / 64);
    if (tiles > 65535) return hipErrorInvalidValue;
    if (a.patch_pos > 0)
        hipLaunchKernelGGL(conv_wgrad_split_kernel<true>, dim3(a.S, tiles, 1), dim3(256), wgrad_split_lds(a.patch_pos), s, a);
    else
        hipLaunchKernelGGL(conv_wgrad_split_kernel<false>, dim3(a.S, tiles, a.k * a.k), dim3(256), wgrad_split_lds(WG_PX), s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const long n = (long)a.Cout * a.Cin * a.k * a.k;
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a.part, a.dw, n, a.S, a.accumulate);
    return hipGetLastError();
}

// ===========================================================================
// Phase-decomposed 2x-upsampling 3x3 convolution, DUAL-PHASE form (included by lns_kernels.hip).
//
// conv3_bf16x3_kernel<.., NTAP = 4> gives every output phase of a source tile its own block.  Here ONE block takes one
// source tile, one ROW phase pa and BOTH column phases pb = 0, 1: the K loop is the per-phase form's (8-channel stages, a
// double-buffered [patch | slab] in LDS, the staging of stage c+1 and the prefetch of stage c+2 interleaved with the MFMAs,
// one barrier per stage), but the patch is gathered, transformed, split and staged ONCE per stage for the two phases, the
// slab is the two phases' slabs side by side (contiguous in the host pack: [cout tile][stage][phase]), and a stage carries
// 24 MFMAs per wave instead of 12.  Per k-step a wave issues the per-phase form's MFMAs for pb = 0, then for pb = 1, each
// into that phase's own acc_hi / acc_lo: the sequence of products into any one accumulator is exactly the per-phase
// form's, the prologue and epilogue arithmetic is the same, so every output element has the same bits (op-level variant 21
// against 17, tests/test_up2_dual_gpu.py).
// A lane then holds the output pixels (2i + pa, 2j) and (2i + pa, 2j + 1) of its couts: ONE 8-byte store per (cout, lane),
// 32 lanes write 256 contiguous bytes (the per-phase form: two blocks each write every other dword of the line).  The
// residual is read the same way.  GroupNorm tile partials: the two slots the two per-phase blocks write, each from that
// phase's values in the per-phase order (convb_tile_stats, scratch in halves of 32 channels).
// Budget: accumulators 2 phases x (hi, lo) x 2 x 16 = 128 registers, at most 256 per wave; LDS 2 x (patch <= 8.2 KB +
// 16 KB) = 49 KB + tables -- two blocks per CU.  Fragments are read per (k-step, phase) HALF-step, one set of 24 registers:
// with a second set read ahead the kernel spilled 13 registers.
//   LDS: 2 x [patch (PP1 units of [8 ch hi | 8 ch lo], halves swizzled: convf_hi_half) | slab pb 0 | slab pb 1] | tables
// ===========================================================================
#define CONVUD_SLAB 8192           // one (stage, phase) weight slab of a 64-cout tile

size_t convud_lds_bytes(const ConvArgs& a) {
    const size_t pp1 = (size_t)a.PH * a.PW + 1;
    // (the epilogue's statistics scratch, 32 x 133 floats + the masks, reuses the stage buffers)
    const size_t stage = std::max(2 * (pp1 * 32 + 2 * (size_t)CONVUD_SLAB), (size_t)32 * 133 * 4 + 64);
    return stage + ((size_t)a.Cin_pad * 2 + 64) * 4 + 16 + 16;
}
// Per-layer rule (a.up2 != 0 on entry): planar tensors, one patch unit per thread, no fused 1x1, the sample's output inside
// one buffer descriptor, an even output width (a lane's pixel pair never straddles a row; multi-dword buffer accesses need
// dword alignment only).
bool convud_fits(const ConvArgs& a) {
    return a.ks == 3 && a.stride == 1 && a.dil == 1 && a.up2 && a.wb != nullptr && a.Cin_pad >= 8 && (a.Cin_pad % 8) == 0 &&
           (long)a.PH * a.PW <= 256 && !a.x_oct && !a.y_oct && a.w2 == nullptr && (a.Wout & 1) == 0 &&
           (long)a.Cout * a.Hout * a.Wout * 4 < (1L << 31) && convud_lds_bytes(a) <= 80 * 1024;
}

__global__ __launch_bounds__(256, 2) void conv3_up2d_kernel(ConvArgs a) {
    constexpr int NTHR = 256, TM = 64, KC = 8, MT = 2, UB = 32, SLAB = CONVUD_SLAB;
    constexpr int NWU = 2 * SLAB / 16 / NTHR;             // weight 16-byte units per thread per stage (4: one per half-step)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int PH = a.PH, PW = a.PW, PLANE = PH * PW, PP1 = PLANE + 1;
    const int xb_bytes = PP1 * UB;
    const int buf_bytes = xb_bytes + 2 * SLAB;
    char* lds = smem;                                                  // 2 x [Xb | Wb pb 0 | Wb pb 1]
    float* ssl = reinterpret_cast<float*>(lds + 2 * buf_bytes);        // [Cin_pad][2]
    float* addv = ssl + a.Cin_pad * 2;                                 // [64] bias + per-sample add of this cout tile
    unsigned* wmax = reinterpret_cast<unsigned*>(addv + 64);           // [4] per-wave share of the activation bound

    const int tid = threadIdx.x, lane = tid & 63, wn = tid >> 6;
    const int l31 = lane & 31, kh = lane >> 5;
    const int b = blockIdx.y + a.b0;
    int bid = blockIdx.x, ct, pa;
    // XCD-aware order of the per-phase form: blocks g, g + 8, g + 16, ... share an XCD, so the two row phases (x cout tiles)
    // of one source tile are consecutive WITHIN an XCD when the sample's tiles fill whole groups of 8
    if (((a.tiles_x * a.tiles_y) & 7) == 0) {
        const int x = bid & 7, q = bid >> 3, per = 2 * a.cout_tiles;
        const int inner = q % per;
        ct = inner % a.cout_tiles; pa = inner / a.cout_tiles;
        bid = (q / per) * 8 + x;
    } else {
        ct = bid % a.cout_tiles; bid /= a.cout_tiles;
        pa = bid & 1; bid >>= 1;
    }
    const int tx = bid % a.tiles_x, ty = bid / a.tiles_x;
    const int BW = 1 << a.bw_log2, BH = 128 >> a.bw_log2;
    const int HWin = a.Hin * a.Win;
    const float* xb = a.x + (long)b * a.x_bs;
    const bool has_ss = a.ss != nullptr || a.gn_part != nullptr;
    const int pro_mode = has_ss ? (a.act_in == ACT_SWISH ? 2 : 1) : 0;
    LNS_TS_DECL
    LNS_TSTAMP(0)

    // this thread's patch unit: source offset (or none), LDS slot of its hi term (lo: ^ 16); threads past the end of the
    // patch stage into the sink unit
    unsigned udm;
    int uslot;
    float uok;
    {
        const int p = tid, pc = p < PLANE ? p : 0;
        const int py = pc / PW, px = pc - py * PW;
        const int qy = ty * BH + py, qx = tx * BW + px;
        int sy, sx;
        if (a.map_arith) {
            int uy = qy - a.map_pad[0], ux = qx - a.map_pad[1];
            if (uy < 0) uy = a.map_circ[0] ? uy + a.Hin : -1; else if (uy >= a.Hin) uy = a.map_circ[0] ? uy - a.Hin : -1;
            if (ux < 0) ux = a.map_circ[1] ? ux + a.Win : -1; else if (ux >= a.Win) ux = a.map_circ[1] ? ux - a.Win : -1;
            sy = qy < a.map_ext[0] ? uy : -1;
            sx = qx < a.map_ext[1] ? ux : -1;
        } else {
            sy = a.rowmap[qy];
            sx = a.colmap[qx];
        }
        const bool ok = p < PLANE && sy >= 0 && sx >= 0;
        udm = ok ? (unsigned)(sy * a.Win + sx) * 4u : 0u;
        uok = ok ? 1.0f : 0.0f;                          // times the activation scale once the bound is known
        const int slot = p < PLANE ? p : PLANE;
        uslot = slot * UB + convf_hi_half(slot);
    }
    float xinv = 1.0f;
    // [cout tile][stage][phase] slabs: the two column phases of row phase pa are 2 x SLAB contiguous bytes of every stage
    const int ns = a.Cin_pad / KC;
    const char* wslab = reinterpret_cast<const char*>(a.wb) + (long)ct * ns * 4 * SLAB + (long)pa * 2 * SLAB;
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(xb), 0, a.Cin * HWin * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(wslab), 0, (ns * 4 - 2 * pa) * SLAB, 0x00020000);

    // per-lane operand offsets (bytes).  K of one MFMA = 2 taps x 8 channels: lane half kh takes tap 2j + kh = (row j,
    // column kh) of the phase's 2 x 2 source neighbourhood, rows {i - 1 + pa, i + pa} x columns {j - 1 + pb, j + pb}
    int bhi[2][2], aoff[2];           // [pb][j]: the hi term of the B fragment inside a patch buffer (lo: ^ 16)
    {
        const int p = wn * 32 + l31;
        const int boff = ((p >> a.bw_log2) * PW + (p & (BW - 1))) * UB;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            aoff[j] = ((2 * j + kh) * TM + l31) * 16;
#pragma unroll
            for (int pb = 0; pb < 2; ++pb) {
                const int off = boff + ((j + pa) * PW + kh + pb) * UB;
                bhi[pb][j] = off + convf_hi_half(off / UB);
            }
        }
    }

    f32x16 acc_hi[2][MT], acc_lo[2][MT];                  // [pb][mt]
#pragma unroll
    for (int pb = 0; pb < 2; ++pb)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc_hi[pb][mt][r] = 0.0f; acc_lo[pb][mt][r] = 0.0f; }

    float pv[KC];                     // raw prefetched patch values (stage + 2 while in flight)
    unsigned hq[4], lq[4];            // split + packed channel pairs of the stage being written
    u32x4 wq[NWU];

    const int cin_m1 = a.Cin - 1, hw4 = HWin * 4;
    // a padded pixel reads pixel 0 and is multiplied by 0 later; a channel past Cin reads the last channel and meets zero weights
    auto load_pair = [&](int cp, int c0) __attribute__((always_inline)) {
#pragma unroll
        for (int e = 0; e < 2; ++e)
            pv[2 * cp + e] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(xr, (int)udm, min(c0 + 2 * cp + e, cin_m1) * hw4, 0));
    };
    auto split_pair = [&](auto mode_tag, int cp, int c0) __attribute__((always_inline)) {
        constexpr int MODE = decltype(mode_tag)::value;
        float t[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            float v = pv[2 * cp + e];
            if (MODE >= 1) { const float2 st = *reinterpret_cast<const float2*>(ssl + 2 * (c0 + 2 * cp + e)); v = v * st.x + st.y; }
            if (MODE == 2) v = swish_fast(v);
            t[e] = v * uok;
        }
        split2_pair_f16(t[0], t[1], hq[cp], lq[cp]);
    };
    auto flush_unit = [&](char* Xn) __attribute__((always_inline)) {
        *reinterpret_cast<uint4*>(Xn + uslot) = make_uint4(hq[0], hq[1], hq[2], hq[3]);
        *reinterpret_cast<uint4*>(Xn + (uslot ^ 16)) = make_uint4(lq[0], lq[1], lq[2], lq[3]);
    };
    auto load_w = [&](int i, int c0) __attribute__((always_inline)) {
        wq[i] = __builtin_amdgcn_raw_buffer_load_b128(wr, (tid + i * NTHR) * 16, (c0 >> 3) * (4 * SLAB), 0);
    };
    auto write_w = [&](int i, char* Wn) __attribute__((always_inline)) {
        *reinterpret_cast<u32x4*>(Wn + (tid + i * NTHR) * 16) = wq[i];
    };
    // fragments of half-step h = 2j + pb: A[split][mt] (couts of phase pb's slab), B[split] (pixels)
    auto load_frags = [&](int h, const char* Xs, const char* Ws, uint4 (&af)[2][MT], uint4 (&bf)[2]) __attribute__((always_inline)) {
        const int j = h >> 1, pb = h & 1;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
                af[s][mt] = *reinterpret_cast<const uint4*>(Ws + pb * SLAB + s * (4 * TM * 16) + mt * (32 * 16) + aoff[j]);
            bf[s] = *reinterpret_cast<const uint4*>(Xs + (s ? bhi[pb][j] ^ 16 : bhi[pb][j]));
        }
    };

    auto k_loop = [&](auto mode_tag) __attribute__((always_inline)) {
        const int last = a.Cin_pad - KC;
#pragma unroll
        for (int cp = 0; cp < 4; ++cp) load_pair(cp, 0);
#pragma unroll
        for (int i = 0; i < NWU; ++i) load_w(i, 0);
        {
            float addreg = 0.0f;
            if (tid < TM) {
                const int co = ct * TM + tid, cc = co < a.Cout ? co : 0;
                addreg = (a.bias ? a.bias[cc] : 0.0f) + (a.badd ? a.badd[(long)b * a.Cout + cc] : 0.0f);
            }
            stage_ss_bound(a, b, ssl, wmax, tid, NTHR);    // behind the first stage's patch and weight loads
            if (tid < TM) addv[tid] = addreg;
        }
        __syncthreads();                                   // ssl / addv / wmax visible
        LNS_TSTAMP(1)
        uok *= f16x2_scale(block_bound(a, wmax), xinv);    // activations are staged times the sample's power-of-two scale
#pragma unroll
        for (int cp = 0; cp < 4; ++cp) split_pair(mode_tag, cp, 0);
        flush_unit(lds);
#pragma unroll
        for (int i = 0; i < NWU; ++i) write_w(i, lds + xb_bytes);
        {
            const int c1 = KC < last ? KC : last;
#pragma unroll
            for (int cp = 0; cp < 4; ++cp) load_pair(cp, c1);
#pragma unroll
            for (int i = 0; i < NWU; ++i) load_w(i, c1);
        }
        __syncthreads();
        LNS_TSTAMP(2)
        int buf = 0;
        for (int c0 = 0; c0 < a.Cin_pad; c0 += KC) {
            const char* Xs = lds + buf * buf_bytes;
            const char* Ws = Xs + xb_bytes;
            char* Xn = lds + (buf ^ 1) * buf_bytes;
            char* Wn = Xn + xb_bytes;
            const int cw = c0 + KC < last ? c0 + KC : last;
            const int cl2 = c0 + 2 * KC < last ? c0 + 2 * KC : last;
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                // one set of fragments (24 registers): a second set, read a half-step ahead as the per-phase form does, does
                // not fit beside 128 accumulator registers without spilling; the CU's other block covers the LDS latency
                uint4 A[2][MT], Bq[2];
                load_frags(h, Xs, Ws, A, Bq);
                // the per-phase form's order inside a k-step: hh', hl', lh', consecutive MFMAs into different accumulators
#define LNS_UD3(ACC, SA, SB)                                                                                   \
    _Pragma("unroll") for (int mt = 0; mt < MT; ++mt)                                                          \
        ACC[h & 1][mt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, A[SA][mt]),          \
                                                                __builtin_bit_cast(f16x8, Bq[SB]), ACC[h & 1][mt], 0, 0, 0);
                LNS_UD3(acc_hi, 0, 0)
                LNS_UD3(acc_lo, 0, 1)
                LNS_UD3(acc_lo, 1, 0)
#undef LNS_UD3
                // this half-step's share of the staging: one channel pair of the patch unit, a quarter of the two slabs
                split_pair(mode_tag, h, cw);
                load_pair(h, cl2);
                write_w(h, Wn);
                load_w(h, cl2);
                if (h == 3) flush_unit(Xn);
                // schedule: the LDS reads of the half-step first (the next half-step's fragments, this pair's table entries),
                // then after each MFMA a few of the half-step's other instructions
                __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);
#pragma unroll
                for (int g = 0; g < 3 * MT; ++g) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // MFMA
                    __builtin_amdgcn_sched_group_barrier(0x002, 6, 0);   // VALU
                    __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);   // VMEM read
                    __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);   // DS write
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            __syncthreads();
            buf ^= 1;
        }
    };
    if (pro_mode == 2) k_loop(std::integral_constant<int, 2>{});
    else if (pro_mode == 1) k_loop(std::integral_constant<int, 1>{});
    else k_loop(std::integral_constant<int, 0>{});

    // ---- epilogue (fp32): the per-phase form's arithmetic on both phases, the pixel pair stored together -----------------
    LNS_TSTAMP(3)
    const int HWo = a.Hout * a.Wout;
    int pix0;                         // flat output pixel (2i + pa, 2j) of this lane, or -1; (2i + pa, 2j + 1) is the next one
    {
        const int p = wn * 32 + l31;
        const int oy = 2 * (ty * BH + (p >> a.bw_log2)) + pa, ox = 2 * (tx * BW + (p & (BW - 1)));
        pix0 = (oy < a.Hout && ox < a.Wout) ? oy * a.Wout + ox : -1;      // (Wout is even: the pair is inside or outside)
    }
    f32x16 v[2][MT][1];
#pragma unroll
    for (int pb = 0; pb < 2; ++pb)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                v[pb][mt][0][r] = ((acc_hi[pb][mt][r] + acc_lo[pb][mt][r]) * a.unscale) * xinv;
    float* yb = y_base(a, b);
    const float* rb = a.res ? a.res + (long)b * a.res_bs : nullptr;
    const int ybytes = a.Cout * HWo * 4;                  // (convud_fits: below 2^31)
    // lane offset of the pixel pair inside a channel plane; a lane without a pixel starts at 2^31 (dropped by the range check)
    const unsigned vo = pix0 >= 0 ? (unsigned)((4 * kh * HWo + pix0) * 4) : 0x80000000u;
    // residual pairs: all loads issued here, behind the epilogue arithmetic; the channel row in the VGPR offset, so that the
    // range check masks the rows of a ragged cout tile (what lies outside reads as zero and is never stored)
    float rv[2][MT][16];
    if (rb) {
        const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(rb), 0, ybytes, 0x00020000);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const unsigned ro = (unsigned)((ct * TM + mt * 32 + (r & 3) + 8 * (r >> 2)) * HWo * 4);
                const u32x2 t = __builtin_amdgcn_raw_buffer_load_b64(rr, (int)(vo + ro), 0, 0);
                rv[0][mt][r] = __uint_as_float(t[0]); rv[1][mt][r] = __uint_as_float(t[1]);
            }
    }
    if (a.bias || a.badd) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float add = addv[mt * 32 + drow(r, kh)];
#pragma unroll
                for (int pb = 0; pb < 2; ++pb) v[pb][mt][0][r] += add;
            }
    }
    if (a.act_out == ACT_GELU) {
#pragma unroll
        for (int pb = 0; pb < 2; ++pb)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) v[pb][mt][0][r] = act_apply(v[pb][mt][0][r], ACT_GELU);
    } else if (a.act_out == ACT_SWISH) {
#pragma unroll
        for (int pb = 0; pb < 2; ++pb)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) v[pb][mt][0][r] = swish_f(v[pb][mt][0][r]);
    }
    if (rb) {
#pragma unroll
        for (int pb = 0; pb < 2; ++pb)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) v[pb][mt][0][r] += rv[pb][mt][r];
    }
    const bool stats = a.stat_part != nullptr;            // block-uniform
    if (stats) __syncthreads();                           // main-loop LDS reads are done: the scratch reuses the stage buffers
    unsigned am = 0u;
    const __amdgpu_buffer_rsrc_t yr = __builtin_amdgcn_make_buffer_rsrc(yb, 0, ybytes, 0x00020000);
    if ((ct + 1) * TM <= a.Cout && __builtin_amdgcn_ballot_w64(pix0 >= 0) == ~0ull) {
        // every element of the wave's tile is stored: the channel row offset in an SGPR
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int so = ((ct * TM + mt * 32 + (r & 3) + 8 * (r >> 2)) * HWo) * 4;     // uniform
                const float v0 = v[0][mt][0][r], v1 = v[1][mt][0][r];
                const u32x2 t = {__float_as_uint(v0), __float_as_uint(v1)};
                __builtin_amdgcn_raw_buffer_store_b64(t, yr, (int)vo, so, LNS_CONV_STORE_AUX);
                am = max(am, max(abs_bits(v0), abs_bits(v1)));
            }
    } else {
        // ragged tile (image edge, or a cout tile past Cout): the hardware range check does the masking -- the channel row
        // goes into the VGPR offset, everything at or past Cout * Hout * Wout * 4 bytes is dropped
        const unsigned nb = (unsigned)ybytes;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const unsigned vr = vo + (unsigned)(((ct * TM + mt * 32 + (r & 3) + 8 * (r >> 2)) * HWo) * 4);
                const float v0 = v[0][mt][0][r], v1 = v[1][mt][0][r];
                const u32x2 t = {__float_as_uint(v0), __float_as_uint(v1)};
                __builtin_amdgcn_raw_buffer_store_b64(t, yr, (int)vr, 0, LNS_CONV_STORE_AUX);
                am = max(am, vr < nb ? max(abs_bits(v0), abs_bits(v1)) : 0u);
            }
    }
    LNS_TSTAMP(4)
    if (stats) {
        float* sb = reinterpret_cast<float*>(lds);
        const int slot = (ty * a.tiles_x + tx) * 4 + 2 * pa;
        convb_tile_stats<MT, 1, true>(a, v[0], pix0, b, ct, kh, l31, tid, sb, slot, 4);
        __syncthreads();                                  // phase 0's second half has been read
        convb_tile_stats<MT, 1, true>(a, v[1], pix0, b, ct, kh, l31, tid, sb, slot + 1, 4);
    }
    if (a.amax_out) amax_publish_block(a.amax_out, b, am, wmax);    // wmax: free since the prologue
    LNS_TS_DUMP
}

hipError_t launch_conv_up2d(const ConvArgs& a, hipStream_t s) {
    if (!convud_fits(a) || !has_act_bound(a)) return hipErrorInvalidValue;
    dim3 grid(a.tiles_x * a.tiles_y * a.cout_tiles * 2, a.B);
    hipLaunchKernelGGL(conv3_up2d_kernel, grid, dim3(256), convud_lds_bytes(a), s, a);
    return hipGetLastError();
}

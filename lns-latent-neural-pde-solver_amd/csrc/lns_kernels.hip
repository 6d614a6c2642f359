// gfx950 (MI355X / CDNA4) kernels of the LNS rollout hot path.
//
// Numerics: every tensor in HBM and every accumulator is fp32.  The dense contractions run on
//   * v_mfma_f32_32x32x2_f32 (exact fp32 products, k-ordered fmaf chain): stride-2 / thin convolutions, attention,
//     the small FABlock GEMMs, and every convolution when LNS_CONV_FP32_MFMA / LNS_CONV1_FP32_MFMA are set;
//   * v_mfma_f32_32x32x16_f16 on SPLIT operands ("f16x2", the default for 3x3 stride-1 and 1x1 convolutions): each
//     fp32 operand, scaled by a power of two, is the sum of two fp16 terms (22 significant bits + sign), the
//     three kept partial products are exact in fp32 and accumulate in fp32.  The activation scale is chosen PER
//     SAMPLE from the running absolute maximum its producer recorded (ConvArgs::amax_in), so the scheme has no
//     fixed input range (see "dynamic activation scale" below);
//   * v_mfma_f32_32x32x16_bf16 on three-term bf16 splits ("bf16x3", 24 bits, range of fp32): FABlock sandwich
//     and the 3x3 fallback (LNS_CONV3_SPLIT=bf16x3).
// Plain bf16/fp16 products are excluded by the 1e-4 rel-L2 parity budget over 64+ autoregressive steps.
//
// 64-lane wavefront conventions used throughout:
//   l31 = lane & 31, kh = lane >> 5
//   A operand (32 x 2):  lane holds A[row l31][k = kh]
//   B operand (2 x 32):  lane holds B[k = kh][col l31]
//   C/D (32 x 32, 16 regs): reg r of lane holds D[row (r&3) + 8*(r>>2) + 4*kh][col l31]
#include <cstdlib>
#include <type_traits>

#include "lns_kernels.h"
#include "lns_knobs.h"
#include "lns_spectrum.h"

namespace lns {

// cache policy of the big output streams (A/B build knobs; 0 plain, 2 nt, 16 sc1): the split-operand conv epilogue's stores and
// the sandwich kernels' plane stores
#ifndef LNS_CONV_STORE_AUX
#define LNS_CONV_STORE_AUX 0
#endif
// non-temporal stores of the fused (3x3 + 1x1) and (1x1 + 1x1) kernels' outputs (A/B build knobs)
#ifndef LNS_NTS_CONV3F
#define LNS_NTS_CONV3F 0
#endif
#ifndef LNS_NTS_CONV1F
#define LNS_NTS_CONV1F 0
#endif
#ifndef LNS_SAND_STORE_AUX
#define LNS_SAND_STORE_AUX 0
#endif
typedef float f32x16 __attribute__((ext_vector_type(16)));

// Exact (erf) GELU without the ~60-instruction library erff: 1 + erf(x) = 2 - erfc(x) for x >= 0 and erfc(|x|) for
// x < 0, with erfc(z) = t exp(-z^2 + P(t)), t = 1 / (1 + z/2) (Chebyshev fit, fractional error < 1.2e-7 everywhere,
// Numerical Recipes erfcc).  One v_rcp, one v_exp, ten FMAs, branch-free; max |error| of the result 7e-8 against the
// fp64 GELU -- closer than the fp32 erf form itself (6.8e-7: its 1 + erf cancels in the negative tail).
__device__ __forceinline__ float gelu_erfc(float v) {
    const float z = fabsf(v) * 0.70710678118654752440f;
    const float t = __builtin_amdgcn_rcpf(fmaf(0.5f, z, 1.0f));
    float p = 0.17087277f;
    p = fmaf(t, p, -0.82215223f);
    p = fmaf(t, p, 1.48851587f);
    p = fmaf(t, p, -1.13520398f);
    p = fmaf(t, p, 0.27886807f);
    p = fmaf(t, p, -0.18628806f);
    p = fmaf(t, p, 0.09678418f);
    p = fmaf(t, p, 0.37409196f);
    p = fmaf(t, p, 1.00002368f);
    p = fmaf(t, p, -1.26551223f);
    const float e = t * __builtin_amdgcn_exp2f(fmaf(-z, z, p) * 1.44269504088896341f);
    return 0.5f * v * (v >= 0.0f ? 2.0f - e : e);
}

__device__ __forceinline__ float act_apply(float v, int act) {
    if (act == ACT_SWISH) return v / (1.0f + expf(-v));
    if (act == ACT_GELU) return gelu_erfc(v);
    if (act == ACT_RELU) return fmaxf(v, 0.0f);
    if (act == ACT_TANH) return tanhf(v);
    if (act == ACT_SIGMOID) return 1.0f / (1.0f + expf(-v));
    return v;
}

template <int CTRL>
__device__ __forceinline__ float dpp_quad(float x) {            // lane permutation inside every quad of lanes
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xf, 0xf, true));
}
__device__ __forceinline__ int drow(int r, int kh) { return (r & 3) + 8 * (r >> 2) + 4 * kh; }

// Sum over the 64 lanes, the same value in every lane.  Called by whole waves only.  Row (16-lane) sums through DPP
// (quad permutes, half-row and row mirrors: register-file moves, no LDS crossbar round trips), then the four row sums
// through v_readlane; fixed order.
__device__ __forceinline__ float wave_sum(float v) {
    v += dpp_quad<0xB1>(v);          // quad_perm [1,0,3,2]
    v += dpp_quad<0x4E>(v);          // quad_perm [2,3,0,1]
    v += dpp_quad<0x141>(v);         // row_half_mirror
    v += dpp_quad<0x140>(v);         // row_mirror
    const int iv = __builtin_bit_cast(int, v);
    const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(iv, 0));
    const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(iv, 16));
    const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(iv, 32));
    const float r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(iv, 48));
    return (r0 + r1) + (r2 + r3);
}

// ---------------------------------------------------------------------------
// Dynamic activation scale of the f16x2 kernels ("amax side channel").
// Every kernel that produces a tensor a split-operand convolution will read records, per sample, the maximum of the
// IEEE bit patterns of |y| (unsigned max == float max for non-negative values; a NaN is the largest pattern and so
// survives; atomicMax is exact and order-independent, so the result does not depend on block scheduling).  The
// consumer turns the maximum -- pushed through its GroupNorm scale/shift prologue as max_c(|s_c| amax + |t_c|) -- into
// a power-of-two scale S with S * bound in [2^14, 2^15).  Scaling by a power of two does not change the bits of the
// fp16 high/low terms while they are normal numbers, so results do not depend on S in that regime.
// ---------------------------------------------------------------------------
__device__ __forceinline__ unsigned abs_bits(float x) { return __float_as_uint(x) & 0x7fffffffu; }
template <int CTRL>
__device__ __forceinline__ unsigned dpp_u(unsigned x) {
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xf, 0xf, true);
}
// max over the 64 lanes (bit patterns of non-negative floats), the same value in every lane; whole waves only
__device__ __forceinline__ unsigned wave_umax(unsigned v) {
    v = max(v, dpp_u<0xB1>(v));
    v = max(v, dpp_u<0x4E>(v));
    v = max(v, dpp_u<0x141>(v));
    v = max(v, dpp_u<0x140>(v));
    const unsigned r0 = (unsigned)__builtin_amdgcn_readlane((int)v, 0), r1 = (unsigned)__builtin_amdgcn_readlane((int)v, 16);
    const unsigned r2 = (unsigned)__builtin_amdgcn_readlane((int)v, 32), r3 = (unsigned)__builtin_amdgcn_readlane((int)v, 48);
    return max(max(r0, r1), max(r2, r3));
}
// amax vectors are [B][LNS_AMAX_SUB]: reader side
__device__ __forceinline__ unsigned amax_load(const unsigned* amax, int b) {
    const unsigned* p = amax + (long)b * LNS_AMAX_SUB;
    unsigned m = 0u;
#pragma unroll
    for (int k = 0; k < LNS_AMAX_SUB; ++k) m = max(m, p[k]);
    return m;
}
// writer side, one atomic per 256-thread BLOCK through 4 words of LDS nobody else touches any more; called by all
// threads of the block at a converged point
__device__ __forceinline__ void amax_publish_block(unsigned* amax, int b, unsigned local, unsigned* red4) {
    const unsigned m = wave_umax(local);
    if ((threadIdx.x & 63) == 0) red4[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned bm = max(max(red4[0], red4[1]), max(red4[2], red4[3]));
        if (bm) atomicMax(amax + (long)b * LNS_AMAX_SUB + (blockIdx.x & (LNS_AMAX_SUB - 1)), bm);
    }
}
// S = 2^(CONVF_TARGET_EXP - e) for bound = m 2^e (1 <= m < 2), clamped to [2^-110, 2^120]; inv = 1 / S.
// Non-finite bound (exponent field 255): S = 2^-110 and the staged values stay non-finite -> NaN results, as in fp32.
__device__ __forceinline__ float f16x2_scale(unsigned bound_bits, float& inv) {
#ifdef LNS_FIXED_ACT_SCALE      // attribution builds only (tools/drift_attribution.sh): round 1's constant activation scale
    inv = 1.0f / (float)(LNS_FIXED_ACT_SCALE);
    return (float)(LNS_FIXED_ACT_SCALE);
#endif
    const int eb = (int)((bound_bits >> 23) & 0xffu);
    int f = 127 + CONVF_TARGET_EXP + 127 - eb;
    f = f < 17 ? 17 : (f > 247 ? 247 : f);
    inv = __uint_as_float((unsigned)(254 - f) << 23);
    return __uint_as_float((unsigned)f << 23);
}
// Block prologue shared by the split-operand kernels: stages this sample's GroupNorm (scale, shift) table into LDS
// (identity for channels without one) and returns each wave's share of bound = max_c(|s_c| amax + |t_c|) through
// wmax[wave] (4 words of LDS); after the block's next barrier block_bound() gives the block-wide value.
// block-wide sum for blockDim.x == 256 through 4 floats of LDS (defined below)
__device__ __forceinline__ float block_sum_256(float v, float* red);
__device__ __forceinline__ float wave_sum(float v);

// GroupNorm folded into the consumer (ConvArgs::gn_part): (scale, shift) of channel c from the producer's per-tile
// partials.  groups == 1: two block-wide sums over all tiles x channels; otherwise (channels per group a power of two
// <= 64) every thread sums its channel over the tiles and the group over its aligned lanes by xor shuffles.  Equal-count
// merge (every partial covers 128 pixels), two-pass like gn_tile_finalize_kernel; all blocks of a sample run the same
// code on the same data, so the table is bit-identical in all of them.  Called by all 256 threads; uses wmax as scratch.
// `active` = false: a thread that only keeps the block's barriers company (the second wave group of conv3_w8_kernel: `tid` is
// the index inside a group of 256, the sums are those of the first group alone -- the bits of a 256-thread block).
__device__ __forceinline__ void stage_ss_from_partials(const ConvArgs& a, int b, float* ssl, unsigned* wmax, int tid, bool active = true) {
    const int C = a.Cin, tiles = a.gn_tiles;
    const float* pb = a.gn_part + (long)b * tiles * C * 2;
    float* red = reinterpret_cast<float*>(wmax);
    const float cnt = a.gn_count ? (float)a.gn_count : 128.0f;     // pixels behind every partial
    if (a.gn_groups == 1 && a.gn_premul) {
        // statistics of x * p (per-sample channel multiplier): mean_c -> p mean_c, M2_c -> p^2 M2_c, scale -> scale * p
        const float* pm = a.gn_premul + (long)b * C;
        const int E = tiles * C;
        float sm = 0.0f;
        for (int i = tid; active && i < E; i += 256) sm += pm[i % C] * pb[2 * i];
        const float mean = block_sum_256(sm, red) / (float)E;
        float m2 = 0.0f;
        for (int i = tid; active && i < E; i += 256) { const float p = pm[i % C], d = p * pb[2 * i] - mean; m2 += p * p * pb[2 * i + 1] + cnt * d * d; }
        const float var = block_sum_256(m2, red) / (cnt * (float)E);
        const float rstd = 1.0f / sqrtf(var + a.gn_eps);
        for (int c = tid; active && c < a.Cin_pad; c += 256) {
            float2 st = make_float2(1.0f, 0.0f);
            if (c < C) {
                const float ga = a.gn_gamma ? a.gn_gamma[c] : 1.0f, be = a.gn_beta ? a.gn_beta[c] : 0.0f;
                st = make_float2(rstd * ga * pm[c], be - mean * rstd * ga);
            }
            *reinterpret_cast<float2*>(ssl + 2 * c) = st;
        }
    } else if (a.gn_groups == 1) {
        const int E = tiles * C;
        float sm = 0.0f;
        for (int i = tid; active && i < E; i += 256) sm += pb[2 * i];
        const float mean = block_sum_256(sm, red) / (float)E;
        float m2 = 0.0f;
        for (int i = tid; active && i < E; i += 256) { const float d = pb[2 * i] - mean; m2 += pb[2 * i + 1] + cnt * d * d; }
        const float var = block_sum_256(m2, red) / (cnt * (float)E);
        const float rstd = 1.0f / sqrtf(var + a.gn_eps);
        for (int c = tid; active && c < a.Cin_pad; c += 256) {
            float2 st = make_float2(1.0f, 0.0f);
            if (c < C) {
                const float ga = a.gn_gamma ? a.gn_gamma[c] : 1.0f, be = a.gn_beta ? a.gn_beta[c] : 0.0f;
                st = make_float2(rstd * ga, be - mean * rstd * ga);
            }
            *reinterpret_cast<float2*>(ssl + 2 * c) = st;
        }
    } else {
        const int cg = C / a.gn_groups;                    // power of two <= 64: a group is an aligned run of lanes
        for (int c0 = 0; c0 < a.Cin_pad; c0 += 256) {
            const int c = c0 + tid;
            const bool live = active && c < C;
            float sm = 0.0f;
            if (live) for (int t = 0; t < tiles; ++t) sm += pb[((long)t * C + c) * 2];
            for (int o = 1; o < cg; o <<= 1) sm += __shfl_xor(sm, o);
            const float mean = sm / (float)(tiles * cg);
            float m2 = 0.0f;
            if (live) for (int t = 0; t < tiles; ++t) { const float* pp = pb + ((long)t * C + c) * 2; const float d = pp[0] - mean; m2 += pp[1] + cnt * d * d; }
            for (int o = 1; o < cg; o <<= 1) m2 += __shfl_xor(m2, o);
            const float rstd = 1.0f / sqrtf(m2 / (cnt * (float)(tiles * cg)) + a.gn_eps);
            if (active && c < a.Cin_pad) {
                float2 st = make_float2(1.0f, 0.0f);
                if (live) {
                    const float ga = a.gn_gamma ? a.gn_gamma[c] : 1.0f, be = a.gn_beta ? a.gn_beta[c] : 0.0f;
                    st = make_float2(rstd * ga, be - mean * rstd * ga);
                }
                *reinterpret_cast<float2*>(ssl + 2 * c) = st;
            }
        }
    }
    __syncthreads();                                       // (wmax is written again by the caller)
}

// table = false (1x1 kernels without a prologue): `ssl` has no storage, only the bound is published
__device__ __forceinline__ void stage_ss_bound(const ConvArgs& a, int b, float* ssl, unsigned* wmax, int tid, int nthr, bool table = true) {
    if (a.gn_part) {                                       // folded GroupNorm: its output bound is a layer constant
        stage_ss_from_partials(a, b, ssl, wmax, tid);
        return;
    }
    const bool has_ss = a.ss != nullptr;
    if (!table) {                                          // identity prologue: bound = max |x| of the sample
        if (!a.bound_final && (tid & 63) == 0)
            wmax[tid >> 6] = abs_bits(a.amax_in ? __uint_as_float(amax_load(a.amax_in, b)) : a.amax_in_const);
        return;
    }
    if (a.bound_final) {                                   // the bound is a launch constant: only stage the table
        for (int c = tid; c < a.Cin_pad; c += nthr) {
            float2 st = make_float2(1.0f, 0.0f);
            if (has_ss && c < a.Cin) st = *reinterpret_cast<const float2*>(a.ss + ((long)b * a.Cin + c) * 2);
            *reinterpret_cast<float2*>(ssl + 2 * c) = st;
        }
        return;
    }
    const float amax = a.amax_in ? __uint_as_float(amax_load(a.amax_in, b)) : a.amax_in_const;
    unsigned loc = 0u;
    for (int c = tid; c < a.Cin_pad; c += nthr) {
        float2 st = make_float2(1.0f, 0.0f);
        if (has_ss && c < a.Cin) st = *reinterpret_cast<const float2*>(a.ss + ((long)b * a.Cin + c) * 2);
        *reinterpret_cast<float2*>(ssl + 2 * c) = st;
        if (c < a.Cin) loc = max(loc, abs_bits(fmaf(fabsf(st.x), amax, fabsf(st.y))));
    }
    loc = wave_umax(loc);
    if ((tid & 63) == 0) wmax[tid >> 6] = loc;
}
__device__ __forceinline__ unsigned block_bound(const ConvArgs& a, const unsigned* wmax) {
    if (a.bound_final) return __float_as_uint(a.amax_in_const);
    return max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3]));
}

// batch base of the output tensor (two-level addressing for step-batched launches, see ConvArgs::y_bdiv)
__device__ __forceinline__ float* y_base(const ConvArgs& a, int b) {
    if (a.y_bdiv > 0) return a.y + (long)(b % a.y_bdiv) * a.y_bs + (long)(b / a.y_bdiv) * a.y_bs2;
    return a.y + (long)b * a.y_bs;
}

// block-wide sum for blockDim.x == 256 (4 waves); red must hold >= 4 floats
__device__ __forceinline__ float block_sum_256(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// ===========================================================================
// Convolution: implicit GEMM, D[cout][pixel] = W[cout][k] * im2col(X)[k][pixel]
//   - weights are the MFMA A operand (rows = couts), activations the B operand
//     (cols = pixels): output rows land in registers, output pixels on lanes, so
//     every store instruction writes 128-byte contiguous NCHW row segments;
//   - per K stage (KC input channels) the input patch is staged in LDS with the
//     producer's GroupNorm scale/shift + Swish applied on the fly.  3x3: haloed
//     patch, padding / circular wrap / nearest-upsample resolved through row/col
//     index maps (never materialised).  1x1: the image is a flat pixel array, a
//     stage is KC contiguous pixel runs, loaded 16 B per lane when HW % 4 == 0;
//   - software pipeline: while the MFMAs of stage c run out of LDS buffer c&1 the
//     global loads of stage c+1 (patch + weight slab) are in flight into
//     registers; they are transformed and written to the other buffer afterwards
//     -> ONE barrier per stage, global latency hidden behind MFMA;
//   - K order: stage-major (KC fixed per kernel size, see conv_pick_kc_log2),
//     tap-major inside a stage, channel pairs (k = 2*kk + kh).
// ===========================================================================
#define CONV_MAXE3 9    // 3x3: scalar patch elements per thread per 4-channel stage
#define CONV_MAXE3_K8 11 // 3x3: ... per 8-channel stage
#define CONV_MAXE1 16   // 1x1: floats per thread per stage (4 x float4 when vectorised)
#define CONV_MAXW 5     // weight float4 per thread per stage

__device__ __forceinline__ float swish_f(float v) { return v / (1.0f + expf(-v)); }
// prologue Swish inside the K loop: v_exp_f32 + v_rcp_f32 (~1 ulp each; worst-case relative error
// of the result ~3e-7 for |v| <= 5, far below the accumulation noise of the following 576-term sums)
__device__ __forceinline__ float swish_fast(float v) {
    const float e = __builtin_amdgcn_exp2f(v * -1.44269504088896341f);
    return v * __builtin_amdgcn_rcpf(1.0f + e);
}

// KCL = channels per LDS stage (3x3: 4 or 8, 1x1: 16).  The MFMA loop always walks a stage in
// sub-stages of KORD channels (3x3: 4, 1x1: 16), tap-major inside a sub-stage, so the fp32
// accumulation ORDER of an output is the same for every KCL / tile variant / batch.
// FUSE2: a second, 1x1 convolution (TM -> TM channels, bias) is applied to the tile in the epilogue
// (needs WGM == 1 and Cout == TM, i.e. every wave holds all channels of its pixels).
template <int MT, int NT, int WGM, int WGN, int KS, bool VEC, int KCL, bool FUSE2 = false>
__global__ __launch_bounds__(64 * WGM * WGN, (MT * NT >= 8 ? 1 : 2)) void conv_mfma_kernel(ConvArgs a) {
    constexpr int NTHR = 64 * WGM * WGN;
    constexpr int TM = WGM * MT * 32;
    constexpr int TN = WGN * NT * 32;
    constexpr int V4 = TM / 4;
    constexpr int KORD = KS == 3 ? 4 : 16;
    constexpr int MAXE = KS == 3 ? (KCL == 8 ? CONV_MAXE3_K8 : CONV_MAXE3) : CONV_MAXE1;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    constexpr int KC = KCL;
    constexpr int KC_LOG2 = KCL == 4 ? 2 : (KCL == 8 ? 3 : 4);
    const int PH = a.PH, PW = a.PW;
    const int PLANE = KS == 3 ? PH * PW : TN;
    constexpr int NW = (KS * KS * KCL * TM / 4 + NTHR - 1) / NTHR;   // weight float4 per thread per stage
    // LDS stage buffers are sized by the per-thread slot counts, so every slot is written
    // unconditionally (no per-element branches in the K loop)
    constexpr int xs_floats = MAXE * NTHR;
    constexpr int ws_floats = NW * NTHR * 4;
    constexpr int buf_floats = xs_floats + ws_floats;
    float* lds = reinterpret_cast<float*>(smem);           // 2 x [Xs | Ws]
    float* ssl = lds + 2 * buf_floats;                     // [Cin_pad][2] scale/shift of this sample
    int* rmap = reinterpret_cast<int*>(ssl + a.Cin_pad * 2);
    int* cmap = rmap + PH;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, kh = lane >> 5;
    const int wm = wave / WGN, wn = wave % WGN;

    const int b = blockIdx.y + a.b0;
    int bid = blockIdx.x;
    const int ct = bid % a.cout_tiles;
    bid /= a.cout_tiles;
    const int tx = bid % a.tiles_x;
    const int ty = bid / a.tiles_x;
    const int BW = 1 << a.bw_log2;
    const int BH = TN >> a.bw_log2;
    const int HWin = a.Hin * a.Win;
    const float* xb = a.x + (long)b * a.x_bs;
    const bool has_ss = a.ss != nullptr;
    const int pro_mode = has_ss ? (a.act_in == ACT_SWISH ? 2 : 1) : 0;   // prologue: none / scale-shift / + Swish

    for (int i = tid; i < a.Cin_pad * 2; i += NTHR)
        ssl[i] = (has_ss && i < a.Cin * 2) ? a.ss[(long)b * a.Cin * 2 + i] : ((i & 1) ? 0.0f : 1.0f);
    if (KS == 3) {
        for (int i = tid; i < PH; i += NTHR) rmap[i] = a.rowmap[ty * BH * a.stride + i];
        for (int i = tid; i < PW; i += NTHR) cmap[i] = a.colmap[tx * BW * a.stride + i];
    }
    __syncthreads();

    // ---- per-thread patch descriptors (the same in every stage) ----------------
    // 3x3   : source offset inside a stage (-1 = zero) | channel-in-stage << 24, one per element
    // 1x1   : one descriptor per 4 consecutive pixels (VEC) or per pixel
    constexpr int NDESC = KS == 3 ? MAXE : (VEC ? CONV_MAXE1 / 4 : CONV_MAXE1);
    int pdesc[NDESC];
    const int p0 = tx * TN;   // 1x1: first flat pixel of this tile
    if (KS == 3) {
        const int total = KC * PLANE;
        int r = tid / PW, cx = tid - r * PW;                 // r = cl*PH + py
        const int r_step = NTHR / PW, c_step = NTHR - r_step * PW;
#pragma unroll
        for (int j = 0; j < NDESC; ++j) {
            int d = -1;
            if (tid + j * NTHR < total) {
                const int cl = a.ph_magic ? (int)__umulhi((unsigned)r, a.ph_magic) : r;   // r / PH
                const int py = r - cl * PH;
                const int sy = rmap[py];
                const int sx = cmap[cx];
                if (sy >= 0 && sx >= 0) d = (cl * HWin + sy * a.Win + sx) | (cl << 24);
            }
            pdesc[j] = d;
            cx += c_step; r += r_step;
            if (cx >= PW) { cx -= PW; ++r; }
        }
    } else {
        constexpr int PER = VEC ? TN / 4 : TN;               // descriptors per channel
#pragma unroll
        for (int j = 0; j < NDESC; ++j) {
            const int idx = tid + j * NTHR;
            const int cl = idx / PER, pp = (idx - cl * PER) * (VEC ? 4 : 1);
            pdesc[j] = (cl < KC && p0 + pp < HWin) ? ((cl * HWin + p0 + pp) | (cl << 24)) : -1;
        }
    }
    // per-thread weight slab descriptors (float offset of the stage-0 source)
    const int nw4 = KS * KS * KC * V4;
    int wdesc[NW];
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        const int fi = tid + i * NTHR;
        const int row = fi / V4, c4 = fi - row * V4;
        const int tap = row >> KC_LOG2, k = row & (KC - 1);
        wdesc[i] = (fi < nw4) ? ((tap * a.Cin_pad + k) * a.Cout_pad + ct * TM + c4 * 4) : 0;   // clamped: slot unused
    }

    int boff[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int p = (wn * NT + nt) * 32 + l31;
        boff[nt] = KS == 3 ? ((p >> a.bw_log2) * a.stride) * PW + (p & (BW - 1)) * a.stride : p;
    }

    f32x16 acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.0f;

    float pv[MAXE];
    float wv[NW][4];

    // ---- staging slots ---------------------------------------------------------
    // slot q < NDESC : patch descriptor q ; slot NDESC + i : weight float4 i.
    // load_slot : global -> registers (unconditional; masked elements read the sample's first
    //             floats, always in bounds, and are zeroed at write time)
    // write_slot: registers -> LDS with the prologue transform (MODE: 0 none, 1 scale/shift,
    //             2 scale/shift + Swish); every slot is written, so no branches.
    auto load_slot = [&](int q, int c0) __attribute__((always_inline)) {
        if (q < NDESC) {
            const int d = pdesc[q];
            const bool ok = d >= 0 && (c0 + (d >> 24)) < a.Cin;
            const float* src = ok ? xb + ((long)c0 * HWin + (d & 0xFFFFFF)) : xb;
            if (KS == 1 && VEC) {
                const float4 t = *reinterpret_cast<const float4*>(src);
                pv[4 * q + 0] = t.x; pv[4 * q + 1] = t.y; pv[4 * q + 2] = t.z; pv[4 * q + 3] = t.w;
            } else {
                pv[q] = *src;
            }
        } else {
            const int i = q - NDESC;
            const float4 t = *reinterpret_cast<const float4*>(a.w + ((long)c0 * a.Cout_pad + wdesc[i]));
            wv[i][0] = t.x; wv[i][1] = t.y; wv[i][2] = t.z; wv[i][3] = t.w;
        }
    };
    auto write_slot = [&](auto mode_tag, int q, int c0, float* Xs, float* Ws) __attribute__((always_inline)) {
        constexpr int MODE = decltype(mode_tag)::value;
        if (q < NDESC) {
            const int d = pdesc[q];
            const int c = c0 + ((d >> 24) & 63);
            const bool ok = d >= 0 && c < a.Cin;
            float2 st = make_float2(1.0f, 0.0f);
            if (MODE >= 1) st = *reinterpret_cast<const float2*>(ssl + 2 * (c < a.Cin_pad ? c : 0));
            if (KS == 1 && VEC) {
                float4 t;
                float* tp = &t.x;
#if defined(LNS_PKEXP) && LNS_PKEXP >= 1
                // Co-residency experiment (tools/pk_experiment.sh; built WITH packed-fp32 ops, never shipped): this is the
                // victim's x * s + t whose SLP-vectorised form -- two v_pk_fma_f32 reading (s, t) through op_sel, the
                // second one overwriting the (s, t) pair -- returned shift 0.0 for a quarter of a wave beside a 16-bit
                // MFMA kernel.  1: four scalar v_fma_f32 (the vectoriser is fenced off); 2: the packed pair by hand, every
                // destination a fresh register pair (early clobber: no aliasing with the op_sel source); 3: the packed
                // pair by hand with the compiler's register assignment (second destination = the (s, t) pair).
                typedef float pk2 __attribute__((ext_vector_type(2)));
                float fv[4];
                if (MODE >= 1) {
#if LNS_PKEXP == 1
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        float v = fmaf(pv[4 * q + u], st.x, st.y);
                        asm volatile("" : "+v"(v));
                        fv[u] = v;
                    }
#else
                    pk2 sp = {st.x, st.y};
                    const pk2 i0 = {pv[4 * q + 0], pv[4 * q + 1]}, i1 = {pv[4 * q + 2], pv[4 * q + 3]};
                    pk2 o0, o1;
                    asm volatile("v_pk_fma_f32 %0, %1, %2, %2 op_sel:[0,0,1] op_sel_hi:[1,0,1]" : "=&v"(o0) : "v"(i0), "v"(sp));
#if LNS_PKEXP == 2
                    asm volatile("v_pk_fma_f32 %0, %1, %2, %2 op_sel:[0,0,1] op_sel_hi:[1,0,1]" : "=&v"(o1) : "v"(i1), "v"(sp));
#else
                    asm volatile("v_pk_fma_f32 %0, %1, %0, %0 op_sel:[0,0,1] op_sel_hi:[1,0,1]" : "+v"(sp) : "v"(i1));
                    o1 = sp;
#endif
                    fv[0] = o0[0]; fv[1] = o0[1]; fv[2] = o1[0]; fv[3] = o1[1];
#endif
                } else {
#pragma unroll
                    for (int u = 0; u < 4; ++u) fv[u] = pv[4 * q + u];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    float v = fv[u];
                    if (MODE == 2) v = swish_fast(v);
                    tp[u] = ok ? v : 0.0f;
                }
#else
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    float v = pv[4 * q + u];
                    if (MODE >= 1) v = v * st.x + st.y;
                    if (MODE == 2) v = swish_fast(v);
                    tp[u] = ok ? v : 0.0f;
                }
#endif
                *reinterpret_cast<float4*>(Xs + (tid + q * NTHR) * 4) = t;
            } else {
                float v = pv[q];
                if (MODE >= 1) v = v * st.x + st.y;
                if (MODE == 2) v = swish_fast(v);
                Xs[tid + q * NTHR] = ok ? v : 0.0f;
            }
        } else {
            const int i = q - NDESC;
            *reinterpret_cast<float4*>(Ws + (tid + i * NTHR) * 4) = make_float4(wv[i][0], wv[i][1], wv[i][2], wv[i][3]);
        }
    };

    int toff[KS * KS];
#pragma unroll
    for (int t = 0; t < KS * KS; ++t) toff[t] = KS == 3 ? ((t / 3) * a.dil) * PW + (t % 3) * a.dil : 0;

    // MFMA steps of one stage, in accumulation order: sub-stage (KORD channels) > tap > channel pair
    constexpr int NSUB = KCL / KORD, NKK = KORD / 2, NSTEP = NSUB * KS * KS * NKK;
    constexpr int NSLOT = NDESC + NW;
    constexpr int SPS = (NSLOT + NSTEP - 1) / NSTEP;      // staging slots handled per MFMA step
    auto load_ops = [&](int s, const float* wbase, const float* xbase, float (&av)[MT], float (&bv)[NT])
                        __attribute__((always_inline)) {
        const int sub = s / (KS * KS * NKK), rem = s - sub * (KS * KS * NKK);
        const int t = rem / NKK, kk = rem - t * NKK;
        const int k0 = sub * KORD + 2 * kk;
        const float* wsp = wbase + (t * KC + k0) * TM;
        const float* xsp = xbase + k0 * PLANE + toff[t];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) av[mt] = wsp[mt * 32];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) bv[nt] = xsp[boff[nt]];
    };

    // One K loop per prologue mode (the mode is block-uniform): while the MFMAs of stage c run
    // from LDS buffer c&1, the SAME instruction stream (a) transforms and writes the registers
    // holding stage c+1 into the other buffer and (b) re-fills each register, as soon as it is
    // free, with stage c+2 from global memory.  Staging is spread over the MFMA steps, so the
    // matrix pipe is not idle while a wave stages; one barrier per stage.
    // patch slots actually used by this launch (the compile-time bound covers the largest patch)
    const int nused = KS == 3 ? (KC * PLANE + NTHR - 1) / NTHR
                              : (VEC ? (KC * (TN / 4) + NTHR - 1) / NTHR : (KC * TN + NTHR - 1) / NTHR);
    auto k_loop = [&](auto mode_tag) __attribute__((always_inline)) {
        const int last = a.Cin_pad - KC;
#pragma unroll
        for (int q = 0; q < NSLOT; ++q) load_slot(q, 0);
#pragma unroll
        for (int q = 0; q < NSLOT; ++q) write_slot(mode_tag, q, 0, lds, lds + xs_floats);
#pragma unroll
        for (int q = 0; q < NSLOT; ++q) load_slot(q, KC < last ? KC : last);
        __syncthreads();
        int buf = 0;
        for (int c0 = 0; c0 < a.Cin_pad; c0 += KC) {
            const float* Xs = lds + buf * buf_floats;
            const float* Ws = Xs + xs_floats;
            float* Xn = lds + (buf ^ 1) * buf_floats;
            float* Wn = Xn + xs_floats;
            // past the end the staging repeats the last stage into the idle buffer (harmless, branch-free)
            const int cw = c0 + KC < last ? c0 + KC : last;
            const int cl2 = c0 + 2 * KC < last ? c0 + 2 * KC : last;
            const float* wbase = Ws + wm * (MT * 32) + l31 + kh * TM;
            const float* xbase = Xs + kh * PLANE;
            // operand look-ahead: LA steps of LDS reads are in flight while a step's MFMAs execute
            // (small per-wave tiles have short steps, so they look further ahead)
            constexpr int LA = (MT * NT <= 2) ? 2 : 1;
            float av[LA + 1][MT], bv[LA + 1][NT];
#pragma unroll
            for (int p = 0; p < LA; ++p)
                if (p < NSTEP) load_ops(p, wbase, xbase, av[p], bv[p]);
#pragma unroll
            for (int s = 0; s < NSTEP; ++s) {
                if (s + LA < NSTEP) load_ops(s + LA, wbase, xbase, av[(s + LA) % (LA + 1)], bv[(s + LA) % (LA + 1)]);
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
                        acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s % (LA + 1)][mt], bv[s % (LA + 1)][nt], acc[mt][nt], 0, 0, 0);
#pragma unroll
                for (int u = 0; u < SPS; ++u) {
                    const int q = s * SPS + u;
                    // patch slots beyond this launch's patch size do nothing (uniform skip)
                    if (q < NSLOT && (q >= NDESC || q < nused)) {
                        write_slot(mode_tag, q, cw, Xn, Wn);
                        load_slot(q, cl2);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);   // pin the interleave (and bound register pressure)
            }
            __syncthreads();
            buf ^= 1;
        }
    };
    if (pro_mode == 2) k_loop(std::integral_constant<int, 2>{});
    else if (pro_mode == 1) k_loop(std::integral_constant<int, 1>{});
    else k_loop(std::integral_constant<int, 0>{});

    // ---- epilogue ---------------------------------------------------------------
    const int HWo = a.Hout * a.Wout;
    float* yb = y_base(a, b);
    const float* rb = a.res ? a.res + (long)b * a.res_bs : nullptr;
    const bool full_co = (ct + 1) * TM <= a.Cout;   // no cout masking needed in this block
    if (a.bias || a.badd) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int cob = ct * TM + (wm * MT + mt) * 32 + 4 * kh;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = cob + (r & 3) + 8 * (r >> 2);
                const int cc = co < a.Cout ? co : 0;
                float add = 0.0f;
                if (a.bias) add += a.bias[cc];
                if (a.badd) add += a.badd[(long)b * a.Cout + cc];
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[mt][nt][r] += add;
            }
        }
    }
    if (a.act_out == ACT_GELU) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[mt][nt][r] = act_apply(acc[mt][nt][r], ACT_GELU);
    } else if (a.act_out == ACT_SWISH) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[mt][nt][r] = swish_f(acc[mt][nt][r]);
    }
    // Fused second 1x1 convolution: Y2[co2][px] = sum_co W2[co2][co] * Y1[co][px] + bias2[co2].
    // The accumulator tile Y1 (rows = channels in registers, pixels on lanes) is exactly the B
    // operand layout of the next MFMA when the contraction runs over its ROW index: k-step r of
    // channel block mt takes accumulator register r (lanes kh=0 supply row drow(r,0), kh=1 row
    // drow(r,1)); the A operand W2 (LDS, [k][co2] = the packed 1x1 weight slab) is fetched in the
    // matching permuted k order.  Y1 never leaves registers.
    if (FUSE2) {
        static_assert(!FUSE2 || WGM == 1, "fused 1x1 needs all channels of a pixel in one wave");
        float* W2s = lds;                                   // the stage buffers are free now
        __syncthreads();
        for (int i = tid; i < TM * TM / 4; i += NTHR) {
            const int k = i / (TM / 4), c4 = i - k * (TM / 4);
            *reinterpret_cast<float4*>(W2s + k * TM + c4 * 4) =
                *reinterpret_cast<const float4*>(a.w2 + (long)k * a.Cout2_pad + c4 * 4);
        }
        __syncthreads();
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            f32x16 acc2[MT];
#pragma unroll
            for (int m2 = 0; m2 < MT; ++m2) {
#pragma unroll
                for (int r = 0; r < 16; ++r) acc2[m2][r] = 0.0f;
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        acc2[m2] = __builtin_amdgcn_mfma_f32_32x32x2f32(
                            W2s[(mt * 32 + drow(r, kh)) * TM + m2 * 32 + l31], acc[mt][nt][r], acc2[m2], 0, 0, 0);
            }
#pragma unroll
            for (int m2 = 0; m2 < MT; ++m2)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co2 = m2 * 32 + drow(r, kh);
                    acc[m2][nt][r] = acc2[m2][r] + (a.bias2 ? a.bias2[co2] : 0.0f);
                }
        }
    }
    // stores: row r of a tile is cout cob + (r&3) + 8*(r>>2); 128-byte pixel runs per half-wave.
    // Offsets from one per-(mt,nt) base pointer are multiples of HWo (uniform scalars).
    unsigned am = 0u;                                  // bit pattern of max |stored value| (amax side channel)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int p = (wn * NT + nt) * 32 + l31;
        int oy, ox;
        if (KS == 3) { oy = ty * BH + (p >> a.bw_log2); ox = tx * BW + (p & (BW - 1)); }
        else { oy = 0; ox = p0 + p; }
        const bool pvld = KS == 3 ? ((oy < a.Hout) && (ox < a.Wout)) : (ox < HWo);
        const int pix = oy * a.Wout + ox;
        if (!pvld) continue;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int cob = ct * TM + (wm * MT + mt) * 32 + 4 * kh;
            float* yp = yb + ((long)cob * HWo + pix);
            if (full_co) {
                if (rb) {
                    const float* rp = rb + ((long)cob * HWo + pix);
                    float rr[16];                              // all residual loads in flight before the first store
#pragma unroll
                    for (int r = 0; r < 16; ++r) rr[r] = rp[((r & 3) + 8 * (r >> 2)) * HWo];
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float v = acc[mt][nt][r] + rr[r];
                        yp[((r & 3) + 8 * (r >> 2)) * HWo] = v;
                        am = max(am, abs_bits(v));
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        yp[((r & 3) + 8 * (r >> 2)) * HWo] = acc[mt][nt][r];
                        am = max(am, abs_bits(acc[mt][nt][r]));
                    }
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = cob + (r & 3) + 8 * (r >> 2);
                    if (co < a.Cout) {
                        const int ro = ((r & 3) + 8 * (r >> 2)) * HWo;
                        float v = acc[mt][nt][r];
                        if (rb) v += rb[(long)cob * HWo + pix + ro];
                        yp[ro] = v;
                        am = max(am, abs_bits(v));
                    }
                }
            }
        }
    }
    if (a.amax_out) {                                  // block-uniform
        __syncthreads();                               // every wave is done with the stage buffers
        amax_publish_block(a.amax_out, b, am, reinterpret_cast<unsigned*>(lds));
    }
}

static const ConvVariantInfo kConvInfo[CV_COUNT] = {
    {128, 256}, {64, 256}, {128, 128}, {64, 128}, {64, 64}, {32, 128}};

ConvVariantInfo conv_variant_info(int v) {
    return (v == CV_B32 || v == CV_F32) ? ConvVariantInfo{32, 128} : v == CV_THIN ? ConvVariantInfo{32, 1024}
           : (v == CV_F256 || v == CV_P256) ? ConvVariantInfo{64, 256} : v >= CV_B64 ? ConvVariantInfo{64, 128} : kConvInfo[v];
}

// Stage depth (channels per LDS stage).  It is a function of the kernel size ONLY
// (3x3: 4, 1x1: 16), never of the tile variant or batch: the fp32
// accumulation order of an output element is then independent of how the launch was tiled,
// so a trajectory's result is bit-identical whatever batch (or GPU shard) it is computed in.
int conv_pick_kc_log2(int ks, int stride, int kc_log2_max) {
    (void)stride;
    const bool k4 = knobs().conv_kcl4;   // tuning knob
    int lg = ks == 3 ? (k4 ? 2 : 3) : 4;     // preferred LDS stage depth; conv_fits() may fall back to 4 for 3x3
    return lg < kc_log2_max ? lg : kc_log2_max;
}

static int conv_maxe(int ks, int KC) { return ks == 3 ? (KC == 8 ? CONV_MAXE3_K8 : CONV_MAXE3) : CONV_MAXE1; }

size_t conv_lds_bytes(int variant, const ConvArgs& a) {
    if (cv_is_pc(variant)) return convpc_lds_bytes(a, variant == CV_P256 ? 2 : 1);
    if (cv_is_split_3x3(variant))
        return convb_lds_bytes(a, (variant == CV_B32 || variant == CV_F32) ? 32 : 64, cv_is_f16x2_3x3(variant) ? 2 : 3, 2);
    if (variant == CV_B1) return convb1_lds_bytes(a);
    if (variant == CV_THIN) return 0;
    const int KC = 1 << a.kc_log2;
    const int TM = kConvInfo[variant].TM;
    const size_t xs = (size_t)conv_maxe(a.ks, KC) * 256;
    const size_t ws = (size_t)(((size_t)a.ks * a.ks * KC * TM / 4 + 255) / 256) * 256 * 4;
    return (2 * (xs + ws) + (size_t)a.Cin_pad * 2 + a.PH + a.PW) * 4 + 16;
}

bool conv_fits(int variant, const ConvArgs& a) {
    if (cv_is_pc(variant)) return convpc_geom_fits(a, variant == CV_P256 ? 2 : 1);
    if (cv_is_split_3x3(variant)) return convb_fits(a);
    if (variant == CV_B1) return convb1_fits(a);
    if (variant == CV_THIN) return a.ks == 1 && a.stride == 1;   // pointer-dependent conditions are checked at launch
    const long KC = 1 << a.kc_log2;
    const int TN = kConvInfo[variant].TN;
    if (a.ks == 3 ? (KC != 4 && KC != 8) : (KC != 16)) return false;
    if (conv_lds_bytes(variant, a) > (KC == 8 ? 72 : 150) * 1024 || (a.Cin_pad % KC) != 0) return false;
    if (a.ks == 3) return KC * a.PH * a.PW <= (long)conv_maxe(3, (int)KC) * 256;
    return KC * TN <= (long)CONV_MAXE1 * 256;
}

template <int MT, int NT, int WGM, int WGN>
static hipError_t launch_conv_t(const ConvArgs& a, size_t lds, hipStream_t s) {
    dim3 grid(a.tiles_x * a.tiles_y * a.cout_tiles, a.B);
    dim3 blk(64 * WGM * WGN);
    if (a.w2) {
        if constexpr (WGM == 1 && MT == 2) {
            if (a.ks == 3 && a.kc_log2 == 3) hipLaunchKernelGGL((conv_mfma_kernel<MT, NT, WGM, WGN, 3, false, 8, true>), grid, blk, lds, s, a);
            else if (a.ks == 3) hipLaunchKernelGGL((conv_mfma_kernel<MT, NT, WGM, WGN, 3, false, 4, true>), grid, blk, lds, s, a);
            else if (a.vec4) hipLaunchKernelGGL((conv_mfma_kernel<MT, NT, WGM, WGN, 1, true, 16, true>), grid, blk, lds, s, a);
            else hipLaunchKernelGGL((conv_mfma_kernel<MT, NT, WGM, WGN, 1, false, 16, true>), grid, blk, lds, s, a);
            return hipGetLastError();
        } else {
            return hipErrorInvalidValue;
        }
    }
    if (a.ks == 3 && a.kc_log2 == 3) hipLaunchKernelGGL((conv_mfma_kernel<MT, NT, WGM, WGN, 3, false, 8>), grid, blk, lds, s, a);
    else if (a.ks == 3) hipLaunchKernelGGL((conv_mfma_kernel<MT, NT, WGM, WGN, 3, false, 4>), grid, blk, lds, s, a);
    else if (a.vec4) hipLaunchKernelGGL((conv_mfma_kernel<MT, NT, WGM, WGN, 1, true, 16>), grid, blk, lds, s, a);
    else hipLaunchKernelGGL((conv_mfma_kernel<MT, NT, WGM, WGN, 1, false, 16>), grid, blk, lds, s, a);
    return hipGetLastError();
}

hipError_t launch_conv(int variant, const ConvArgs& a, hipStream_t s) {
    // OCT8 tensors: inputs of the f16x2 3x3 kernels, outputs of the kernels with the shared split-operand epilogue
    if (a.x_oct && !(cv_is_f16x2_3x3(variant) && !cv_is_pc(variant))) return hipErrorInvalidValue;
    if (a.y_oct && !((cv_is_split_3x3(variant) && !cv_is_pc(variant)) || (variant == CV_B1 && a.ct_per_block == 0))) return hipErrorInvalidValue;
    if (cv_is_pc(variant)) return launch_conv_pc(variant == CV_P256 ? 2 : 1, a, s);
    if (cv_is_split_3x3(variant)) return launch_conv_bf16x3(variant, a, s);
    if (variant == CV_B1) return launch_conv1_bf16x3(a, s);
    if (variant == CV_THIN) return launch_conv1_thin(a, s);
    if (!conv_fits(variant, a)) return hipErrorInvalidValue;
    const size_t lds = conv_lds_bytes(variant, a);
    switch (variant) {
        case CV_L128: return launch_conv_t<2, 4, 2, 2>(a, lds, s);
        case CV_L64: return launch_conv_t<2, 2, 1, 4>(a, lds, s);
        case CV_M128: return launch_conv_t<2, 2, 2, 2>(a, lds, s);
        case CV_M64: return launch_conv_t<2, 1, 1, 4>(a, lds, s);
        case CV_S64: return launch_conv_t<1, 1, 2, 2>(a, lds, s);
        case CV_S32: return launch_conv_t<1, 1, 1, 4>(a, lds, s);
    }
    return hipErrorInvalidValue;
}

// ===========================================================================
// 3x3 convolution on the bf16 matrix pipe with fp32-level accuracy ("bf16x3").
// Every fp32 operand x is split into three bf16 terms x = h + m + l (24 significant bits);
// x*y ~= hh' + [hm' + mh' + hl' + lh' + mm'] (the dropped terms are <= 2^-23 |xy|).  bf16 x bf16
// products are exact in fp32 and v_mfma_f32_32x32x16_bf16 accumulates in fp32, so the result
// matches an fp32 GEMM to rounding.  The hh' terms go to one accumulator (the same K-long fp32
// chain as the fp32 kernel), the five small terms to a second one (their rounding errors are
// 2^-8 smaller), summed once in the epilogue.  6 bf16 MFMAs (32 cycles, K=16) replace 8 fp32
// MFMAs (64 cycles, K=2): 2.7x the fp32-MFMA rate.
//   tile  : 64 couts x 128 pixels (NT=1), 4 waves, wave = 64 couts x 32 pixels, 2 waves/SIMD.
//           The 256-pixel shape (NT=2: 344 registers, 1 wave/SIMD, 95 KB LDS) measured slower on
//           every layer mix (15.5k vs 16.4k trajectory-steps/s) and is not instantiated -- see DESIGN.md.
//   stage : 8 input channels; MFMA K=16 = 2 taps x 8 channels (9 taps padded to 10)
//   LDS   : patch  [split][pixel][8 ch] bf16 (16-byte units: conflict-free b128 reads),
//           weights [split][tap 0..8][cout][8 ch] bf16 (straight copy of the host slab); the 10th,
//           non-existent tap of the last k-step reads a shared all-zero patch unit instead
//   same software pipeline as the fp32 kernel (register prefetch two stages ahead, staging
//   interleaved with the MFMA steps, one barrier per stage); prologue transform, padding maps,
//   epilogue (bias / act / fused 1x1 / residual) identical.
// ===========================================================================
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
#define CONVB_MAXU 2      // patch units (pixel x 8 channels) per thread per stage
#define CONVB_NWU 7       // weight 16-byte units per thread per stage (1728 per slab)

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned pk_bf16(float x, float y) {      // v_cvt_pk_bf16_f32 (RNE)
    f32x2 v = {x, y};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
}
// two fp32 values -> packed (h, m, l) bf16 pairs with x = h + m + l to 24 bits
__device__ __forceinline__ void split3_pair(float x, float y, unsigned& h, unsigned& m, unsigned& l) {
    h = pk_bf16(x, y);
    const float rx = x - __uint_as_float(h << 16), ry = y - __uint_as_float(h & 0xffff0000u);
    m = pk_bf16(rx, ry);
    l = pk_bf16(rx - __uint_as_float(m << 16), ry - __uint_as_float(m & 0xffff0000u));
}

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
// two fp32 values -> packed (h, l) fp16 pairs with x = h + l to ~23 bits (RNE: v_cvt_pk_f16_f32)
__device__ __forceinline__ void split2_pair_f16(float x, float y, unsigned& h, unsigned& l) {
    const f32x2 v = {x, y};
    const f16x2 hh = __builtin_convertvector(v, f16x2);
    const f32x2 hb = __builtin_convertvector(hh, f32x2);
    const f32x2 r = {x - hb[0], y - hb[1]};
    h = __builtin_bit_cast(unsigned, hh);
    l = __builtin_bit_cast(unsigned, __builtin_convertvector(r, f16x2));
}

// Diagnostic build (-DLNS_TS): per-block phase timestamps (100 MHz wall clock) of the split-operand kernels, written to
// ConvArgs::dbg_ts [blocks][8]: entry, tables published, loop start, loop end, stores issued, stores acknowledged,
// HW_ID, XCC_ID (tools/ts_analyze.py).  Expands to nothing in the shipped library.
#ifdef LNS_TS
#define LNS_TS_DECL long long ts_[6] = {0, 0, 0, 0, 0, 0};
#if LNS_TS == 3
// -DLNS_TS=3: the clock the chip holds inside the K loop (MI355X_MICROARCH.md, DVFS give-back item 6): the 100 MHz wall clock
// (s_memrealtime) and the shader clock counter (s_memtime) at loop start and loop end; slots 0 / 1 = wall clock, 2 / 3 = shader
// clock.  In-kernel clock = (ts[3] - ts[2]) / (ts[1] - ts[0]) x 100 MHz (tools/clock_analyze.py).
#define LNS_TSTAMP(i) if ((i) == 2 || (i) == 3) { __builtin_amdgcn_sched_barrier(0); ts_[(i) - 2] = wall_clock64(); ts_[i] = (long long)__builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); }
#elif LNS_TS == 2
#define LNS_TSTAMP(i) if ((i) == 5) { __builtin_amdgcn_sched_barrier(0); ts_[i] = wall_clock64(); __builtin_amdgcn_sched_barrier(0); }
#else
#define LNS_TSTAMP(i) { __builtin_amdgcn_sched_barrier(0); ts_[i] = wall_clock64(); __builtin_amdgcn_sched_barrier(0); }
#endif
#define LNS_TS_DUMP                                                                                   \
    __builtin_amdgcn_s_waitcnt(0);                                                                    \
    LNS_TSTAMP(5)                                                                                     \
    if (a.dbg_ts && threadIdx.x == 0) {                                                               \
        long long* d_ = a.dbg_ts + ((long)blockIdx.y * gridDim.x + blockIdx.x) * 8;                   \
        for (int i_ = 0; i_ < 6; ++i_) d_[i_] = ts_[i_];                                              \
        d_[6] = __builtin_amdgcn_s_getreg((31 << 11) | 4);                                            \
        d_[7] = __builtin_amdgcn_s_getreg((31 << 11) | 20);                                           \
    }
#else
#define LNS_TS_DECL
#define LNS_TSTAMP(i)
#define LNS_TS_DUMP
#endif
// -DLNS_TS=2: the six slots are taken INSIDE the epilogue instead (start, after the activation, fused-conv weights in
// LDS, fused conv done, stores issued, statistics done)
#if defined(LNS_TS) && LNS_TS == 2
#define LNS_ETS(i) if (ets) { __builtin_amdgcn_sched_barrier(0); ets[i] = wall_clock64(); __builtin_amdgcn_sched_barrier(0); }
#define LNS_ETS_ARG , ts_
#else
#define LNS_ETS(i)
#define LNS_ETS_ARG , nullptr
#endif

// Shared epilogue of the bf16x3 kernels (64-cout tile, wave = 64 couts x 32*NT pixels): sums the two
// accumulators, then bias / per-sample add / activation / fused second 1x1 conv (fp32 MFMA, the
// accumulator tile as B operand, see conv_mfma_kernel) / residual, and the coalesced stores.
// pix[nt]: flat output pixel of this lane in pixel tile nt, or -1.
// addv: LDS vector [TM] of (bias + per-sample add) of this cout tile, staged in the prologue so that the epilogue
// does not start with a round trip to L2 (null: read bias / badd from global memory here).
// OCT: the OCT8 output / residual paths (ConvArgs::y_oct) are compiled in.  The input-stationary 1x1 form (always a planar
// output: FABlock in_proj feeds the plane-wise sandwich) is at its register budget and leaves them out -- with them the same
// kernel measured 56 instead of 35 us per launch (same-box A/B, gpurun_out/ab_r03).
// SHALF: the tile statistics go through the LDS scratch in two halves of 32 channels (17 KB instead of 34 KB; two more
// barriers): the quad-phase upsampling conv (conv3_up2q.inc) keeps its whole split patch in LDS and has 18.5 KB of scratch.
// NORES: the launch has no residual tensor (host-checked): the 32 registers of the residual tile are not reserved.
// (convb_tile_stats, defined behind the epilogue, is its statistics tail: the dual-phase upsampling conv calls it per phase)
template <int MT, int NT, bool SHALF>
__device__ __forceinline__ void convb_tile_stats(const ConvArgs& a, const f32x16 (&acc)[MT][NT], int pix0, int b, int ct, int kh,
                                                 int l31, int tid, float* sb, int sp_tile, int tile_mult);
template <int NT, bool FUSE2, int MT = 2, bool STATS = true, bool OCT = true, bool SHALF = false, bool NORES = false, bool NTS = false>
__device__ __forceinline__ void convb_epilogue(const ConvArgs& a, f32x16 (&acc_hi)[MT][NT], f32x16 (&acc_lo)[MT][NT],
                                               const int (&pix)[NT], int b, int ct, int kh, int l31, int tid, char* lds,
                                               float xinv, unsigned& am, const float* addv = nullptr, int sp_tile = -1, long long* ets = nullptr,
                                               int tile_mult = 1) {
    constexpr int TM = 32 * MT, NTHR = 256;      // ct counts TM-wide cout tiles
    static_assert(!FUSE2 || MT == 2, "the fused second 1x1 needs all 64 channels of a pixel in one wave");
    // fused second conv: its weights are requested first, so that their L2 latency hides behind the first conv's epilogue
    // arithmetic (they were loaded behind a barrier: 1 of the ~4 us the fused epilogue cost per block)
    LNS_ETS(0)
    float w2v[FUSE2 ? TM * TM / NTHR : 1];
    if (FUSE2) {
#pragma unroll
        for (int u = 0; u < TM * TM / NTHR; ++u) {
            const int i = tid + u * NTHR, k = i / TM, co2 = i - k * TM;      // fp32 pack [k = co1][Cout2_pad]
            w2v[u] = a.w2[(long)k * a.Cout2_pad + co2];
        }
    }
    f32x16 acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r)      // two powers of two (1 / weight scale, 1 / activation scale), applied one after
                acc[mt][nt][r] = ((acc_hi[mt][nt][r] + acc_lo[mt][nt][r]) * a.unscale) * xinv;   // the other: no intermediate underflow
    const int HWo = a.Hout * a.Wout;
    float* yb = y_base(a, b);
    const float* rb = (!NORES && a.res) ? a.res + (long)b * a.res_bs : nullptr;
    // residual tile: all loads issued here, branch-free (clamped addresses), so their latency hides behind the
    // epilogue arithmetic instead of one round trip per stored element (y may alias nothing, but the compiler
    // cannot know and would not move a load above an earlier store)
    float rv[MT][NT][16];
    if (OCT && rb && a.y_oct) {
        // OCT8 residual ([Cout/8][HWo][8], planner: Cout % 8 == 0, tensor < 2 GB): the lane's four consecutive couts of
        // register group g are 16 contiguous bytes; octet row in the VGPR offset so that the range check masks a ragged
        // cout tile, a lane without a pixel starts at 2^31
        const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(rb), 0, a.Cout * HWo * 4, 0x00020000);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const unsigned vo = pix[nt] >= 0 ? (unsigned)(pix[nt] * 32 + kh * 16) : 0x80000000u;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const unsigned ro = (unsigned)(((ct * TM + mt * 32) / 8 + g) * HWo * 32);
                    const u32x4 t = __builtin_amdgcn_raw_buffer_load_b128(rr, (int)(vo + ro), 0, 0);
#pragma unroll
                    for (int j = 0; j < 4; ++j) rv[mt][nt][4 * g + j] = __uint_as_float(t[j]);
                }
        }
    } else if (rb && (long)a.Cout * HWo * 4 < (1L << 31)) {
        // through a buffer descriptor of the sample's residual tensor, addressed like the stores below (lane offset in
        // one VGPR, channel row in the scalar offset); what lies outside the tensor reads as zero and is never stored
        const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(rb), 0, a.Cout * HWo * 4, 0x00020000);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const unsigned vo = pix[nt] >= 0 ? (unsigned)((4 * kh * HWo + pix[nt]) * 4) : 0x80000000u;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = ct * TM + mt * 32 + (r & 3) + 8 * (r >> 2);
                    // a row past Cout must not wrap into range through the scalar offset (it is outside the range check)
                    rv[mt][nt][r] = row + 4 < a.Cout || (ct + 1) * TM <= a.Cout
                                        ? __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rr, (int)vo, row * HWo * 4, 0))
                                        : __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rr, (int)(vo + (unsigned)(row * HWo * 4)), 0, 0));
                }
        }
    } else if (rb) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const int cob = ct * TM + mt * 32 + 4 * kh;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = cob + (r & 3) + 8 * (r >> 2);
                    const bool ok = pix[nt] >= 0 && co < a.Cout;
                    rv[mt][nt][r] = rb[ok ? (long)co * HWo + pix[nt] : 0];      // elements that are not ok are never stored
                }
            }
    }
    if (addv) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float add = addv[mt * 32 + drow(r, kh)];
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[mt][nt][r] += add;
            }
    } else if (a.bias || a.badd) {
        // all loads of one vector issued back to back (no per-element branch, one wait)
        float add[MT][16];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) add[mt][r] = 0.0f;
        if (a.bias) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = ct * TM + mt * 32 + drow(r, kh);
                    add[mt][r] = a.bias[co < a.Cout ? co : 0];
                }
        }
        if (a.badd) {
            const float* bp = a.badd + (long)b * a.Cout;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = ct * TM + mt * 32 + drow(r, kh);
                    add[mt][r] += bp[co < a.Cout ? co : 0];
                }
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[mt][nt][r] += add[mt][r];
    }
    if (a.act_out == ACT_GELU) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[mt][nt][r] = act_apply(acc[mt][nt][r], ACT_GELU);
    } else if (a.act_out == ACT_SWISH) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[mt][nt][r] = swish_f(acc[mt][nt][r]);
    }
    LNS_ETS(1)
    if (FUSE2) {
        // Second 1x1 conv (64 -> 64) on the same split-operand scheme: the accumulator tile Y1 (channels in
        // registers, pixels on lanes) is scaled, split into two fp16 terms IN REGISTERS and is the B operand
        // (k-step t' of channel block mt takes accumulator registers 8t'..8t'+7, i.e. channels
        // mt*32 + 16t' + 4kh + {0..3, 8..11}); W2 is scaled, split and stored in LDS with its input channels
        // permuted inside every 16-block so that those 8 channels are 8 consecutive k positions of the A operand.
        constexpr int W2W = TM + 8;                               // row stride in fp16 elements (16-byte aligned rows)
        unsigned short* W2s = reinterpret_cast<unsigned short*>(lds);   // [2][co2][W2W]
        float* b2s = reinterpret_cast<float*>(W2s + 2 * TM * W2W);      // [TM] bias of the second conv
        __syncthreads();
        {
#pragma unroll
            for (int u = 0; u < TM * TM / NTHR; ++u) {
                const int i = tid + u * NTHR, k = i / TM, co2 = i - k * TM;
                const int w = k & 15;
                const int kp = (k & ~15) | (w & 3) | (((w >> 3) & 1) << 2) | (((w >> 2) & 1) << 3);
                const float wv = w2v[u] * a.w2scale;
                const _Float16 hh = (_Float16)wv;
                const _Float16 ll = (_Float16)(wv - (float)hh);
                W2s[(0 * TM + co2) * W2W + kp] = __builtin_bit_cast(unsigned short, hh);
                W2s[(1 * TM + co2) * W2W + kp] = __builtin_bit_cast(unsigned short, ll);
            }
            if (tid < TM) b2s[tid] = a.bias2 ? a.bias2[tid] : 0.0f;
        }
        __syncthreads();
        LNS_ETS(2)
        const char* w2a = reinterpret_cast<const char*>(W2s) + (l31 * W2W + 8 * kh) * 2;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            // activation scale of the second conv: this wave's own tile maximum (the tile is a function of the sample
            // and the layer geometry only, never of the batch)
            unsigned tm = 0u;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) tm = max(tm, abs_bits(acc[mt][nt][r]));
            float inv2;
            const float s2 = f16x2_scale(wave_umax(tm), inv2);
            const float w2inv = 1.0f / a.w2scale;                     // powers of two
            f32x16 a2h[MT], a2l[MT];
#pragma unroll
            for (int m2 = 0; m2 < MT; ++m2)
#pragma unroll
                for (int r = 0; r < 16; ++r) { a2h[m2][r] = 0.0f; a2l[m2][r] = 0.0f; }
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int tp = 0; tp < 2; ++tp) {
                    unsigned hq[4], lq[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        split2_pair_f16(acc[mt][nt][8 * tp + 2 * e] * s2, acc[mt][nt][8 * tp + 2 * e + 1] * s2, hq[e], lq[e]);
                    const f16x8 bh = __builtin_bit_cast(f16x8, make_uint4(hq[0], hq[1], hq[2], hq[3]));
                    const f16x8 bl = __builtin_bit_cast(f16x8, make_uint4(lq[0], lq[1], lq[2], lq[3]));
#pragma unroll
                    for (int m2 = 0; m2 < MT; ++m2) {
                        const char* wp = w2a + (m2 * 32) * (W2W * 2) + (mt * 32 + 16 * tp) * 2;
                        const f16x8 ah = *reinterpret_cast<const f16x8*>(wp);
                        const f16x8 al = *reinterpret_cast<const f16x8*>(wp + TM * W2W * 2);
                        a2h[m2] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, a2h[m2], 0, 0, 0);
                        a2l[m2] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, a2l[m2], 0, 0, 0);
                        a2l[m2] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, a2l[m2], 0, 0, 0);
                    }
                }
#pragma unroll
            for (int m2 = 0; m2 < MT; ++m2)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    acc[m2][nt][r] = ((a2h[m2][r] + a2l[m2][r]) * w2inv) * inv2 + b2s[m2 * 32 + drow(r, kh)];
        }
    }
    LNS_ETS(3)
    // GroupNorm statistics of the stored tile (planner: only when the 128-pixel tiles cover the plane exactly, so
    // every pixel of the tile is valid): the tile goes through LDS as [channel][pixel], four threads per channel
    // take 32 pixels each (two-pass mean / centred second moment in registers) and merge pairwise (Chan et al.).
    constexpr int SROW = 133;                                    // 128 pixels + one pad word per 32 + 1
    // (STATS = false: kernels the planner never asks for tile statistics -- the input-stationary 1x1 form, which is at its
    //  register budget -- do not carry the code)
    const bool stats = STATS && NT == 1 && a.stat_part != nullptr;     // block-uniform (32-cout tiles: half the threads)
    float* sb = reinterpret_cast<float*>(lds);
    if (stats) __syncthreads();                                  // main-loop / fused-conv LDS reads are done
    // (am: amax side channel, bit pattern of max |stored value|; the calling kernel publishes it once per block)
    // Fast path (wave-uniform): every element of the wave's tile is stored -- no per-element masks or branches.  One
    // buffer store per element: the sample's base in the descriptor, the lane's offset in one VGPR for all 16*MT
    // rows, the channel row offset in an SGPR (the masked loop below costs ~16 instructions and two branches per
    // element; it was 2.4 - 3.5 us of a block's 18 - 34 us lifetime on the 64^2 / 128^2 layers).
    bool lane_ok = true;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) lane_ok = lane_ok && pix[nt] >= 0;
    const long ybytes = (long)a.Cout * HWo * 4;
#ifdef LNS_NO_FAST_STORE
    constexpr bool kFastStore = false;
#else
    constexpr bool kFastStore = true;
#endif
    if (OCT && a.y_oct) {
        // OCT8 output: one 16-byte store per register group (4 per 32-cout block) instead of 16 dword stores; the hardware
        // range check drops lanes without a pixel (offset 2^31) and octet rows past Cout (ragged cout tile)
        const __amdgpu_buffer_rsrc_t yr = __builtin_amdgcn_make_buffer_rsrc(yb, 0, (int)ybytes, 0x00020000);
        const unsigned nb = (unsigned)ybytes;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const unsigned vo = pix[nt] >= 0 ? (unsigned)(pix[nt] * 32 + kh * 16) : 0x80000000u;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const unsigned vr = vo + (unsigned)(((ct * TM + mt * 32) / 8 + g) * HWo * 32);
                    u32x4 t;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        float v = acc[mt][nt][4 * g + j];
                        if (rb) v += rv[mt][nt][4 * g + j];
                        t[j] = __float_as_uint(v);
                        am = max(am, vr < nb ? abs_bits(v) : 0u);
                        if (SHALF) acc[mt][nt][4 * g + j] = v;
                        else if (stats) sb[(mt * 32 + drow(4 * g + j, kh)) * SROW + (tid >> 6) * 33 + l31] = v;     // (masked below)
                    }
                    __builtin_amdgcn_raw_buffer_store_b128(t, yr, (int)vr, 0, 0);
                }
        }
    } else if (kFastStore && (ct + 1) * TM <= a.Cout && ybytes < (1L << 31) && __builtin_amdgcn_ballot_w64(lane_ok) == ~0ull) {
        const __amdgpu_buffer_rsrc_t yr = __builtin_amdgcn_make_buffer_rsrc(yb, 0, (int)ybytes, 0x00020000);
        if (rb) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[mt][nt][r] += rv[mt][nt][r];
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int vo = (4 * kh * HWo + pix[nt]) * 4;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int so = ((ct * TM + mt * 32 + (r & 3) + 8 * (r >> 2)) * HWo) * 4;     // uniform
                    const float v = acc[mt][nt][r];
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), yr, vo, so, NTS ? 2 : LNS_CONV_STORE_AUX);
                    am = max(am, abs_bits(v));
                }
        }
        if (stats && !SHALF) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) sb[(mt * 32 + drow(r, kh)) * SROW + (tid >> 6) * 33 + l31] = acc[mt][nt][r];
        }
    } else if (kFastStore && ybytes < (1L << 31)) {
        // Ragged tile (image edge, or a cout tile past Cout): the same stores with the hardware range check doing the
        // masking -- the channel row goes into the VGPR offset (the range check ignores the scalar offset), a lane
        // without a pixel starts at 2^31, and everything at or past Cout * Hout * Wout * 4 bytes is dropped.
        const __amdgpu_buffer_rsrc_t yr = __builtin_amdgcn_make_buffer_rsrc(yb, 0, (int)ybytes, 0x00020000);
        const unsigned nb = (unsigned)ybytes;
        if (rb) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[mt][nt][r] += rv[mt][nt][r];
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const unsigned vo = pix[nt] >= 0 ? (unsigned)((4 * kh * HWo + pix[nt]) * 4) : 0x80000000u;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const unsigned vr = vo + (unsigned)(((ct * TM + mt * 32 + (r & 3) + 8 * (r >> 2)) * HWo) * 4);
                    const float v = acc[mt][nt][r];
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), yr, (int)vr, 0, NTS ? 2 : LNS_CONV_STORE_AUX);
                    am = max(am, vr < nb ? abs_bits(v) : 0u);
                    if (stats && !SHALF) sb[(mt * 32 + drow(r, kh)) * SROW + (tid >> 6) * 33 + l31] = v;     // (masked below)
                }
        }
    } else
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        if (pix[nt] < 0) continue;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int cob = ct * TM + mt * 32 + 4 * kh;
            float* yp = yb + ((long)cob * HWo + pix[nt]);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = cob + (r & 3) + 8 * (r >> 2);
                if (co < a.Cout) {
                    const int ro = ((r & 3) + 8 * (r >> 2)) * HWo;
                    float v = acc[mt][nt][r];
                    if (rb) v += rv[mt][nt][r];
                    yp[ro] = v;
                    am = max(am, abs_bits(v));
                    if (SHALF) acc[mt][nt][r] = v;
                    else if (stats) sb[(mt * 32 + drow(r, kh)) * SROW + (tid >> 6) * 33 + l31] = v;
                }
            }
        }
    }
    LNS_ETS(4)
    if (stats) convb_tile_stats<MT, NT, SHALF>(a, acc, pix[0], b, ct, kh, l31, tid, sb, sp_tile, tile_mult);
}

// GroupNorm tile partials of one stored tile (the tail of convb_epilogue; the dual-phase upsampling conv, conv3_up2d.inc,
// calls it once per column phase): acc is the final register tile, sb the LDS scratch ([TM][SROW] floats + the masks, or
// [32][SROW] with SHALF), already filled by the caller unless SHALF.  Block-uniform call, every thread of the block.
template <int MT, int NT, bool SHALF>
__device__ __forceinline__ void convb_tile_stats(const ConvArgs& a, const f32x16 (&acc)[MT][NT], int pix0, int b, int ct, int kh,
                                                 int l31, int tid, float* sb, int sp_tile, int tile_mult) {
    constexpr int TM = 32 * MT, SROW = 133;
    constexpr int SROWS = SHALF ? 32 : TM;          // channel rows of the scratch tile per pass
    for (int hf = 0; hf < (SHALF ? MT : 1); ++hf) {
        if (SHALF) {      // this half's 32 channels of the (final) register tile -> scratch
            if (hf) __syncthreads();                 // the previous half has been read
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
                if (mt == hf) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) sb[drow(r, kh) * SROW + (tid >> 6) * 33 + l31] = acc[mt][0][r];
                }
        }
        // ragged single tile (ConvArgs::stat_count valid pixels): which of a wave's 32 pixels exist, one word per wave
        unsigned* smask = reinterpret_cast<unsigned*>(sb + SROWS * SROW);
        const unsigned long long have = __builtin_amdgcn_ballot_w64(pix0 >= 0);     // (all lanes: lanes 0..31 are the wave's pixels)
        if (a.stat_count && (tid & 63) == 0) smask[tid >> 6] = (unsigned)have;
        __syncthreads();
        const int c = tid >> 2, q = tid & 3;
        if (c < SROWS) {         // (whole waves: 64-cout tiles keep all four busy, 32-cout tiles / half passes two)
        const float* row = sb + c * SROW + q * 33;
        float v[32];
#pragma unroll
        for (int i = 0; i < 32; ++i) v[i] = row[i];
        float mean, m2;
        if (a.stat_count) {
            // exact two-pass statistics over the valid pixels: the four threads of a channel add their masked sums (quad
            // permutes; every lane gets the same total), then their masked squared deviations from the common mean
            const unsigned mk = smask[q];
            float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
#pragma unroll
            for (int i = 0; i < 32; i += 4) {
                s0 += (mk >> i) & 1u ? v[i] : 0.0f; s1 += (mk >> (i + 1)) & 1u ? v[i + 1] : 0.0f;
                s2 += (mk >> (i + 2)) & 1u ? v[i + 2] : 0.0f; s3 += (mk >> (i + 3)) & 1u ? v[i + 3] : 0.0f;
            }
            float sm = (s0 + s1) + (s2 + s3);
            sm += dpp_quad<0xB1>(sm);
            sm += dpp_quad<0x4E>(sm);
            // (one ragged tile: the plane's pixel count; ragged tiles of a larger plane: this tile's own valid pixels)
            const float nval = a.stat_count > 0 ? (float)a.stat_count
                                                : (float)(__popc(smask[0]) + __popc(smask[1]) + __popc(smask[2]) + __popc(smask[3]));
            mean = sm / nval;
            float q0 = 0.0f, q1 = 0.0f, q2 = 0.0f, q3 = 0.0f;
#pragma unroll
            for (int i = 0; i < 32; i += 4) {
                const float d0 = v[i] - mean, d1 = v[i + 1] - mean, d2 = v[i + 2] - mean, d3 = v[i + 3] - mean;
                q0 += (mk >> i) & 1u ? d0 * d0 : 0.0f; q1 += (mk >> (i + 1)) & 1u ? d1 * d1 : 0.0f;
                q2 += (mk >> (i + 2)) & 1u ? d2 * d2 : 0.0f; q3 += (mk >> (i + 3)) & 1u ? d3 * d3 : 0.0f;
            }
            m2 = (q0 + q1) + (q2 + q3);
            m2 += dpp_quad<0xB1>(m2);
            m2 += dpp_quad<0x4E>(m2);
        } else {
        float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
#pragma unroll
        for (int i = 0; i < 32; i += 4) { s0 += v[i]; s1 += v[i + 1]; s2 += v[i + 2]; s3 += v[i + 3]; }
        mean = ((s0 + s1) + (s2 + s3)) * (1.0f / 32.0f);
        float q0 = 0.0f, q1 = 0.0f, q2 = 0.0f, q3 = 0.0f;
#pragma unroll
        for (int i = 0; i < 32; i += 4) {
            const float d0 = v[i] - mean, d1 = v[i + 1] - mean, d2 = v[i + 2] - mean, d3 = v[i + 3] - mean;
            q0 += d0 * d0; q1 += d1 * d1; q2 += d2 * d2; q3 += d3 * d3;
        }
        m2 = (q0 + q1) + (q2 + q3);
        {   // 32 + 32 pixels, then 64 + 64 (lanes of one quad: DPP quad_perm, no LDS round trip)
            const float mo = dpp_quad<0xB1>(mean), qo = dpp_quad<0xB1>(m2), d = mean - mo;      // [1,0,3,2]
            m2 = (m2 + qo) + d * d * 16.0f;
            mean = 0.5f * (mean + mo);
        }
        {
            const float mo = dpp_quad<0x4E>(mean), qo = dpp_quad<0x4E>(m2), d = mean - mo;      // [2,3,0,1]
            m2 = (m2 + qo) + d * d * 32.0f;
            mean = 0.5f * (mean + mo);
        }
        }
        const int co = ct * TM + (SHALF ? hf * 32 : 0) + c;
        if (q == 0 && co < a.Cout) {
            const int tile = sp_tile >= 0 ? sp_tile : (int)blockIdx.x / a.cout_tiles, ntiles = a.tiles_x * a.tiles_y * tile_mult;
            float* pp = a.stat_part + (((long)b * ntiles + tile) * a.Cout + co) * 2;
            pp[0] = mean; pp[1] = m2;
        }
        }
    }
}

// f16x2 patch units are 32 bytes ([8 ch hi | 8 ch lo] fp16), one per patch pixel.  At a 32-byte lane stride the lanes l and
// l + 8 of a ds_read_b128 group fall on the same banks (banking: (address / 4) mod 64) -- EVERY B-fragment read was a two-way
// conflict (20 % of the kernel's LDS-array cycles in profiles/r03_pmc.json), and so was every patch write (lanes l, l + 4,
// banking mod 32).  Which 16-byte half of a unit holds the hi term therefore alternates with bits 2 and 3 of the pixel's patch
// index: consecutive pixels then cover all banks in both access shapes (any base offset).  Returns 0 or 16.
// LNS_CONV3_NO_SWIZZLE: A/B build knob.
__device__ __forceinline__ int convf_hi_half(int patch_index) {
#ifdef LNS_CONV3_NO_SWIZZLE
    return 0;
#else
    return (((patch_index >> 2) ^ (patch_index >> 3)) & 1) << 4;
#endif
}

template <int NT, int NU, bool FUSE2, int MT = 2, int SPL = 3, int NTAP = 9, bool XOCT = false>
__global__ __launch_bounds__(256, 1) void conv3_bf16x3_kernel(ConvArgs a) {
    // XOCT: the input tensor is channel-octet-interleaved ([Cin/8][Hin*Win][8] per sample, ConvArgs::x_oct; Cin % 8 == 0):
    // the 8 channels of a K stage of a patch pixel are 32 contiguous bytes -- two 16-byte buffer loads per unit and stage
    // instead of eight dword gathers out of eight channel planes (same values into the same registers: same bits).
    // NTAP = 4: the 3x3 convolution of a 2x nearest-upsampled tensor, PHASE-DECOMPOSED.  Output pixel (2i + pa, 2j + pb)
    // only sees the 2 x 2 source neighbourhood rows {i-1+pa, i+pa} x columns {j-1+pb, j+pb}, with the 3x3 taps that
    // fall on the same source pixel summed on the host (pa = 0: rows {ky 0 | ky 1+2}, pa = 1: {ky 0+1 | ky 2}; columns
    // alike): 4 taps = two K = 16 MFMA steps per 8-channel stage instead of five (nine taps padded to ten) -- 2.5x
    // fewer matrix instructions for the same layer.  A block computes 128 SOURCE pixels of one phase; the patch is the
    // source-resolution halo patch (maps of a plain pad-1 3x3 convolution of the source), the slab is the phase's.
    // (Two accumulators per tile -- hh' apart from hl' + lh' -- are part of the accuracy here: with all three products in
    //  one fp32 accumulator the 64-step NS2d rollout is at 1.0e-4 of the reference instead of 2.7e-5 ... 4.8e-5, and three
    //  blocks per CU at 168 registers spill; measured, not adopted.  The 1x1 kernels, K <= 512, do use one: CONVB1_ONEACC.)
    // SPL = 3: three bf16 terms, six products.  SPL = 2: two fp16 terms of the operand scaled by a power of two
    // (activations x the sample's dynamic scale in the staging, weights per layer on the host), three products hh' + (hl' + lh'); the
    // dropped ll' term is <= 2^-24 |xy|.  Half the MFMAs and 2/3 of the LDS bytes at the accuracy of an fp32 chain.
    // MT = 1: 32-cout tiles (half a weight slab per block).  Same accumulation order, so the planner may pick it
    // freely; it is used when 64-cout tiles would leave CUs with fewer than two blocks.
    constexpr int NTHR = 256, TM = 32 * MT, TN = 128 * NT, KC = 8, NJ = (NTAP + 1) / 2;
    constexpr bool UP2 = NTAP == 4;
    static_assert(NTAP == 9 || (NTAP == 4 && SPL == 2 && MT == 2), "phase form: f16x2, 64-cout tiles");
    constexpr int SLAB64 = SPL * NTAP * 64 * 16;          // host slab of a 64-cout tile, one stage (one phase)
    constexpr int SLAB = SLAB64 * MT / 2;                 // bytes of weights per stage in LDS
    constexpr int NWU = (SLAB / 16 + NTHR - 1) / NTHR;    // weight 16-byte units per thread per stage
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int PH = a.PH, PW = a.PW;
    const int PLANE = PH * PW;
    const int PP1 = PLANE + 1;                         // units per buffer; unit PLANE = write sink
    constexpr int UB = SPL * 16;                       // a unit = one patch pixel: [split][8 ch] 16-bit, the splits side by side
    const int xb_bytes = PP1 * UB;                     //  (immediate offsets between them; 32-byte lane stride: conflict-free reads)
    const int buf_bytes = xb_bytes + SLAB;
    char* lds = smem;                                                  // 2 x [Xb | Wb]
    char* zunit = lds + 2 * buf_bytes;                              // one all-zero unit
    float* ssl = reinterpret_cast<float*>(zunit + UB);                 // [Cin_pad][2]
    float* addv = ssl + a.Cin_pad * 2;                                 // [64] bias + per-sample add of this cout tile
    unsigned* wmax = reinterpret_cast<unsigned*>(addv + 64);           // [4] per-wave share of the activation bound

    const int tid = threadIdx.x, lane = tid & 63, wn = tid >> 6;
    const int l31 = lane & 31, kh = lane >> 5;
    const int b = blockIdx.y + a.b0;
    int bid = blockIdx.x;
    int ct, phase = 0;
    if (UP2) {
        // XCD-aware order: blocks g, g + 8, g + 16, ... share an XCD (and its L2), so the four phases (x cout tiles) of one
        // source tile are made consecutive WITHIN an XCD: they read the same source patch (one HBM fetch instead of
        // four) and their stride-2 stores complete each other's 128-byte lines in the same L2 (measured before: 271 MB
        // fetched and 541 MB written per launch of the fused 128^2 layer, for 67 MB of input and 268 MB of output)
        // Only when the sample's tiles fill whole groups of 8 (else most XCDs would idle: 16 x 16 sources have 2 tiles).
        if (((a.tiles_x * a.tiles_y) & 7) == 0) {
            const int x = bid & 7, q = bid >> 3, per = 4 * a.cout_tiles;
            const int inner = q % per;
            ct = inner % a.cout_tiles; phase = inner / a.cout_tiles;
            bid = (q / per) * 8 + x;
        } else {
            ct = bid % a.cout_tiles; bid /= a.cout_tiles;
            phase = bid & 3; bid >>= 2;
        }
    } else {
        ct = bid % a.cout_tiles;
        bid /= a.cout_tiles;
    }
    const int pa = phase >> 1, pb = phase & 1;
    const int tx = bid % a.tiles_x, ty = bid / a.tiles_x;
    const int BW = 1 << a.bw_log2, BH = TN >> a.bw_log2;
    const int HWin = a.Hin * a.Win;
    const float* xb = a.x + (long)b * a.x_bs;
    const bool has_ss = a.ss != nullptr || a.gn_part != nullptr;
    // prologue: none / scale-shift / + Swish / + exact GELU (the conditional propagator's cond_conv1: GroupNorm -> GELU -> conv)
    const int pro_mode = has_ss ? (a.act_in == ACT_SWISH ? 2 : (a.act_in == ACT_GELU ? 3 : 1)) : 0;
    LNS_TS_DECL
    LNS_TSTAMP(0)

    // Prologue: everything the first stage needs is requested from global memory up front -- the row/column source
    // maps of this thread's patch units (direct loads, no LDS round trip), the GroupNorm scale/shift table and the
    // epilogue's add vector (to LDS) -- so the block pays ONE memory latency before its first patch loads, and the
    // epilogue none.
    unsigned udm[NU];                 // byte offset of the unit's source pixel inside a channel plane (zero-extended lane
    int uslot[NU];                    //  offset + uniform channel base = the scalar-base form of the global load)
    float uok[NU];
    {
        int sy[NU], sx[NU];
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int p = tid + u * NTHR;
            const int pc = p < PLANE ? p : 0;
            const int py = pc / PW, px = pc - py * PW;
            const int qy = ty * BH * a.stride + py, qx = tx * BW * a.stride + px;
            if (a.map_arith) {       // (uniform) the planner's build_axis_map() without resize, in registers
                int uy = qy - a.map_pad[0], ux = qx - a.map_pad[1];
                if (uy < 0) uy = a.map_circ[0] ? uy + a.Hin : -1; else if (uy >= a.Hin) uy = a.map_circ[0] ? uy - a.Hin : -1;
                if (ux < 0) ux = a.map_circ[1] ? ux + a.Win : -1; else if (ux >= a.Win) ux = a.map_circ[1] ? ux - a.Win : -1;
                sy[u] = qy < a.map_ext[0] ? uy : -1;
                sx[u] = qx < a.map_ext[1] ? ux : -1;
            } else {
                sy[u] = a.rowmap[qy];
                sx[u] = a.colmap[qx];
            }
        }
        if (tid < UB / 4) reinterpret_cast<unsigned*>(zunit)[tid] = 0u;
        // patch units: unit u = pixel (tid + u*256) of the patch; spatial source offset or none.
        // Threads past the end of the patch stage into the sink unit, so the K loop has no branches.
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int p = tid + u * NTHR;
            const bool ok = p < PLANE && sy[u] >= 0 && sx[u] >= 0;
            udm[u] = ok ? (unsigned)(sy[u] * a.Win + sx[u]) * (XOCT ? 32u : 4u) : 0u;
            uok[u] = ok ? 1.0f : 0.0f;                          // times the activation scale once the bound is known
            uslot[u] = (p < PLANE ? p : PLANE) * UB;
            if (SPL == 2) uslot[u] += convf_hi_half(p < PLANE ? p : PLANE);     // byte offset of the unit's HI term (lo: ^ 16)
        }
    }
    // (the scale/shift table, the add vector and the activation bound are staged inside k_loop, BEHIND the first
    //  stage's patch and weight loads: their memory latencies overlap, and the barrier that publishes them comes after)
    float xinv = 1.0f;
    // weight slab of this cout tile: host slabs hold 64 couts per (split, tap) row; a 32-cout block copies its half
    // of every row.  16 bytes per thread-slot.
    const long wstage = UP2 ? 4L * SLAB64 : SLAB64;    // phase form: [cout tile][stage][phase] slabs
    const char* wslab = reinterpret_cast<const char*>(a.wb) + (long)(ct * MT / 2) * (a.Cin_pad / KC) * wstage +
                        (UP2 ? (long)phase * SLAB64 : 0) + (MT == 1 ? (ct & 1) * 512 : 0);

    // Both operand streams are read through buffer descriptors: lane offset in ONE VGPR, the stage's channel / slab offset
    // in an SGPR -- no 64-bit vector address arithmetic in the K loop (the flat form cost a v_lshl_add_u64 per load).
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(xb), 0, a.Cin * HWin * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(wslab), 0,
                                                                        (int)((a.Cin_pad / KC) * wstage), 0x00020000);

    // per-lane operand offsets (bytes).  K of one MFMA = 2 taps x 8 channels: lane half kh takes tap 2j+kh.
    // The 10th tap does not exist: in k-step 4 the kh=1 lanes multiply the shared zero unit with tap 8's
    // (finite) weights.
    int boff[NT], ltoff[NJ], aoff[NJ];
    int bhi[NT][NJ], blo[NT][NJ];     // f16x2: byte offsets of the hi / lo terms of (pixel tile nt, tap pair j) inside a patch buffer
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int p = (wn * NT + nt) * 32 + l31;
        boff[nt] = (((p >> a.bw_log2) * a.stride) * PW + (p & (BW - 1)) * a.stride) * UB;
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int t = 2 * j + kh;
        const int tc = t < NTAP ? t : NTAP - 1;
        ltoff[j] = UP2 ? (((tc >> 1) + pa) * PW + (tc & 1) + pb) * UB : (((tc / 3) * a.dil) * PW + (tc % 3) * a.dil) * UB;
        aoff[j] = (tc * TM + l31) * 16;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int off = boff[nt] + ltoff[j];
            bhi[nt][j] = SPL == 2 ? off + convf_hi_half(off / UB) : off;
            blo[nt][j] = bhi[nt][j] ^ 16;
        }
    }
    const bool ztap = kh != 0;                          // nine taps: in k-step 4 this lane half reads the zero unit

    f32x16 acc_hi[MT][NT], acc_lo[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc_hi[mt][nt][r] = 0.0f; acc_lo[mt][nt][r] = 0.0f; }

    float pv[NU][KC];                 // raw prefetched patch values (stage + 2 while in flight)
    unsigned hq[NU][4], mq[NU][4], lq[NU][4];   // split + packed channel pairs of the stage being written
    float wq[NWU][4];

    // channel pair cp (channels 2cp, 2cp+1 of a stage) of unit u: global -> registers.
    // Straight-line code (no per-element branches, so the scheduler can interleave it with MFMAs):
    // a padded pixel reads pixel 0 and is multiplied by 0 later; a channel past Cin reads the last channel
    // (finite data) and meets zero weights.
    const int cin_m1 = a.Cin - 1, hw4 = HWin * 4;
    auto load_pair = [&](int u, int cp, int c0) __attribute__((always_inline)) {
        if (XOCT) {
            // OCT8: channel pairs (0, 1) and (2, 3) of a stage arrive together, by ONE 16-byte load issued when the later pair
            // of the half is asked for (its registers are free by then: both pairs of the previous stage have been split)
            if (cp & 1) {
                const u32x4 t = __builtin_amdgcn_raw_buffer_load_b128(xr, (int)udm[u] + 8 * (cp - 1), (c0 >> 3) * (hw4 * 8), 0);
#pragma unroll
                for (int e = 0; e < 4; ++e) pv[u][2 * (cp - 1) + e] = __uint_as_float(t[e]);
            }
            return;
        }
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int c = c0 + 2 * cp + e;
            pv[u][2 * cp + e] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(xr, (int)udm[u], min(c, cin_m1) * hw4, 0));
        }
    };
    // prologue transform + 3-way split of one channel pair
    auto split_pair = [&](auto mode_tag, int u, int cp, int c0) __attribute__((always_inline)) {
        constexpr int MODE = decltype(mode_tag)::value;
        float t[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            float v = pv[u][2 * cp + e];
            if (MODE >= 1) { const float2 st = *reinterpret_cast<const float2*>(ssl + 2 * (c0 + 2 * cp + e)); v = v * st.x + st.y; }
            if (MODE == 2) v = swish_fast(v);
            if (MODE == 3) v = gelu_erfc(v);
            t[e] = v * uok[u];
        }
        if (SPL == 3) split3_pair(t[0], t[1], hq[u][cp], mq[u][cp], lq[u][cp]);
        else split2_pair_f16(t[0], t[1], hq[u][cp], mq[u][cp]);
    };
    // the same with the pair's (scale, shift) table entries already in registers: in the main loop they are read
    // from LDS one k-step ahead (together with the next k-step's fragments), so that no MFMA of a k-step sits behind
    // an s_waitcnt for a read issued in that same k-step
    auto split_pair_r = [&](auto mode_tag, int u, int cp, const float4& st) __attribute__((always_inline)) {
        constexpr int MODE = decltype(mode_tag)::value;
        float v0 = pv[u][2 * cp], v1 = pv[u][2 * cp + 1];
        if (MODE >= 1) { v0 = v0 * st.x + st.y; v1 = v1 * st.z + st.w; }
        if (MODE == 2) { v0 = swish_fast(v0); v1 = swish_fast(v1); }
        if (MODE == 3) { v0 = gelu_erfc(v0); v1 = gelu_erfc(v1); }
        v0 *= uok[u]; v1 *= uok[u];
        if (SPL == 3) split3_pair(v0, v1, hq[u][cp], mq[u][cp], lq[u][cp]);
        else split2_pair_f16(v0, v1, hq[u][cp], mq[u][cp]);
    };
    auto flush_unit = [&](int u, char* Xn) __attribute__((always_inline)) {
        if (SPL == 2) {      // swizzled halves (convf_hi_half): uslot is the hi term's slot, the lo term's is the other half
            *reinterpret_cast<uint4*>(Xn + uslot[u]) = make_uint4(hq[u][0], hq[u][1], hq[u][2], hq[u][3]);
            *reinterpret_cast<uint4*>(Xn + (uslot[u] ^ 16)) = make_uint4(mq[u][0], mq[u][1], mq[u][2], mq[u][3]);
            return;
        }
        char* dst = Xn + uslot[u];
        *reinterpret_cast<uint4*>(dst) = make_uint4(hq[u][0], hq[u][1], hq[u][2], hq[u][3]);
        *reinterpret_cast<uint4*>(dst + 16) = make_uint4(mq[u][0], mq[u][1], mq[u][2], mq[u][3]);
        if (SPL == 3) *reinterpret_cast<uint4*>(dst + 32) = make_uint4(lq[u][0], lq[u][1], lq[u][2], lq[u][3]);
    };
    auto load_w = [&](int i, int c0) __attribute__((always_inline)) {
        const int idx = tid + i * NTHR;                  // 16-byte unit inside the slab
        const int off = idx < SLAB / 16 ? idx : SLAB / 16 - 1;
        const unsigned src = MT == 1 ? (off >> 5) * 1024 + (off & 31) * 16 : off * 16;     // row of 64 couts -> its 32
        const u32x4 t = __builtin_amdgcn_raw_buffer_load_b128(wr, (int)src, (c0 >> 3) * (int)wstage, 0);
        wq[i][0] = __uint_as_float(t[0]); wq[i][1] = __uint_as_float(t[1]); wq[i][2] = __uint_as_float(t[2]); wq[i][3] = __uint_as_float(t[3]);
    };
    auto write_w = [&](int i, char* Wn) __attribute__((always_inline)) {
        const int idx = tid + i * NTHR;                  // the last slot's tail rewrites the slab's last unit
        const int off = idx < SLAB / 16 ? idx : SLAB / 16 - 1;
        *reinterpret_cast<float4*>(Wn + (long)off * 16) = make_float4(wq[i][0], wq[i][1], wq[i][2], wq[i][3]);
    };

    // fragments of k-step j: A[s][mt] (couts), B[s][nt] (pixels), s = h / m / l
    auto load_frags = [&](int j, const char* Xs, const char* Ws, uint4 (&af)[SPL][MT], uint4 (&bf)[SPL][NT])
                          __attribute__((always_inline)) {
#pragma unroll
        for (int s = 0; s < SPL; ++s) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
                af[s][mt] = *reinterpret_cast<const uint4*>(Ws + s * (NTAP * TM * 16) + mt * (32 * 16) + aoff[j]);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                if (SPL == 2) {
                    const char* p = Xs + (s ? blo[nt][j] : bhi[nt][j]);
                    if (j == NJ - 1 && (NTAP & 1)) p = ztap ? zunit : p;       // (both halves of the zero unit are zero)
                    bf[s][nt] = *reinterpret_cast<const uint4*>(p);
                } else {
                    const char* p = Xs + boff[nt] + ltoff[j];
                    if (j == NJ - 1 && (NTAP & 1)) p = ztap ? zunit : p;
                    bf[s][nt] = *reinterpret_cast<const uint4*>(p + s * 16);
                }
            }
        }
    };

    // One K loop per prologue mode.  Stage = 8 channels; per k-step 6*MT*NT MFMAs.  The staging of
    // stage c+1 (registers -> LDS, with the transform and split) and the prefetch of stage c+2
    // (global -> registers) are cut into per-k-step pieces (one channel pair per unit, two weight
    // slots) and interleaved with the MFMAs by scheduling groups, so the matrix pipe keeps running
    // while a wave stages; one barrier per stage.
    auto k_loop = [&](auto mode_tag) __attribute__((always_inline)) {
        const int last = a.Cin_pad - KC;
#pragma unroll
        for (int u = 0; u < NU; ++u)
#pragma unroll
            for (int cp = 0; cp < 4; ++cp) load_pair(u, cp, 0);
#pragma unroll
        for (int i = 0; i < NWU; ++i) load_w(i, 0);
        {
            float addreg = 0.0f;
            if (tid < TM) {
                const int co = ct * TM + tid, cc = co < a.Cout ? co : 0;
                addreg = (a.bias ? a.bias[cc] : 0.0f) + (a.badd ? a.badd[(long)b * a.Cout + cc] : 0.0f);
            }
            stage_ss_bound(a, b, ssl, wmax, tid, NTHR);
            if (tid < TM) addv[tid] = addreg;
        }
        __syncthreads();                                   // ssl / addv / wmax / zunit visible
        LNS_TSTAMP(1)
        if (SPL == 2) {   // fp16 split: activations are staged multiplied by the sample's power-of-two scale
            const float xs = f16x2_scale(block_bound(a, wmax), xinv);
#pragma unroll
            for (int u = 0; u < NU; ++u) uok[u] *= xs;
        }
#pragma unroll
        for (int u = 0; u < NU; ++u) {
#pragma unroll
            for (int cp = 0; cp < 4; ++cp) split_pair(mode_tag, u, cp, 0);
            flush_unit(u, lds);
        }
#pragma unroll
        for (int i = 0; i < NWU; ++i) write_w(i, lds + xb_bytes);
        {
            const int c1 = KC < last ? KC : last;
#pragma unroll
            for (int u = 0; u < NU; ++u)
#pragma unroll
                for (int cp = 0; cp < 4; ++cp) load_pair(u, cp, c1);
#pragma unroll
            for (int i = 0; i < NWU; ++i) load_w(i, c1);
        }
        __syncthreads();
        LNS_TSTAMP(2)
        int buf = 0;
        constexpr int MODE = decltype(mode_tag)::value;
        // (scale, shift) of channel pair 0 of stage 1, the first pair the loop transforms
        float4 stq = MODE >= 1 ? *reinterpret_cast<const float4*>(ssl + 2 * (KC < last ? KC : last)) : make_float4(1.f, 0.f, 1.f, 0.f);
        for (int c0 = 0; c0 < a.Cin_pad; c0 += KC) {
            const char* Xs = lds + buf * buf_bytes;
            const char* Ws = Xs + xb_bytes;
            char* Xn = lds + (buf ^ 1) * buf_bytes;
            char* Wn = Xn + xb_bytes;
            const int cw = c0 + KC < last ? c0 + KC : last;
            const int cl2 = c0 + 2 * KC < last ? c0 + 2 * KC : last;
            uint4 af[2][SPL][MT], bf[2][SPL][NT];
#if defined(LNS_KNOCK) && (LNS_KNOCK & 2)     // ... no fragment reads either (one set read once per stage)
            load_frags(0, Xs, Ws, af[0], bf[0]);
            load_frags(1, Xs, Ws, af[1], bf[1]);
#else
            load_frags(0, Xs, Ws, af[0], bf[0]);
#endif
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
#if !(defined(LNS_KNOCK) && (LNS_KNOCK & 2))
                if (j + 1 < NJ) load_frags(j + 1, Xs, Ws, af[(j + 1) & 1], bf[(j + 1) & 1]);
#endif
                // this k-step transforms pair j of stage cw with the table entries read one k-step ago; the entries of
                // the next pair to be transformed (pair j+1, or pair 0 of the following stage) are requested now
                const float4 stu = stq;
                if (!UP2 && MODE >= 1 && j != 3) stq = *reinterpret_cast<const float4*>(ssl + 2 * (j < 3 ? cw + 2 * (j + 1) : cl2));
                auto& A = af[j & 1];
                auto& Bq = bf[j & 1];
                // product-major order: consecutive MFMAs belong to different accumulators
#define LNS_BX3(ACC, SA, SB)                                                                          \
    _Pragma("unroll") for (int mt = 0; mt < MT; ++mt)                                                 \
        _Pragma("unroll") for (int nt = 0; nt < NT; ++nt)                                             \
            ACC[mt][nt] = SPL == 3 ? __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, A[SA][mt]),          \
                                         __builtin_bit_cast(bf16x8, Bq[SB][nt]), ACC[mt][nt], 0, 0, 0)                       \
                                   : __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, A[SA][mt]),            \
                                         __builtin_bit_cast(f16x8, Bq[SB][nt]), ACC[mt][nt], 0, 0, 0);
                if (SPL == 3) {
                    LNS_BX3(acc_lo, 1, 1)
                    LNS_BX3(acc_hi, 0, 0)
                    LNS_BX3(acc_lo, 0, SPL - 1)
                    LNS_BX3(acc_lo, SPL - 1, 0)
                    LNS_BX3(acc_lo, 0, 1)
                    LNS_BX3(acc_lo, 1, 0)
                } else {
                    LNS_BX3(acc_hi, 0, 0)
                    LNS_BX3(acc_lo, 0, 1)
                    LNS_BX3(acc_lo, 1, 0)
                }
#undef LNS_BX3
#if defined(LNS_KNOCK) && (LNS_KNOCK & 1)     // timing what-if (garbage results): no staging inside the K loop
                if (false) {
#else
                if (UP2) {       // two k-steps per stage: two channel pairs and half of the (small) slab each
#endif
#pragma unroll
                    for (int u = 0; u < NU; ++u)
#pragma unroll
                        for (int cp = 2 * j; cp < 2 * j + 2; ++cp) {
                            split_pair(mode_tag, u, cp, cw);
                            load_pair(u, cp, cl2);
                        }
#pragma unroll
                    for (int i = j * ((NWU + 1) / 2); i < (j + 1) * ((NWU + 1) / 2); ++i)
                        if (i < NWU) {
                            write_w(i, Wn);
                            load_w(i, cl2);
                        }
                    if (j == NJ - 1) {
#pragma unroll
                        for (int u = 0; u < NU; ++u) flush_unit(u, Xn);
                    }
#if defined(LNS_KNOCK) && (LNS_KNOCK & 1)
                } else if (false) {
#else
                } else if (j < 4) {
#endif
#pragma unroll
                    for (int u = 0; u < NU; ++u) {
                        split_pair_r(mode_tag, u, j, stu);
                        load_pair(u, j, cl2);
                    }
#pragma unroll
                    for (int i = 2 * j; i < 2 * j + 2; ++i)
                        if (i < NWU) {
                            write_w(i, Wn);
                            load_w(i, cl2);
                        }
                } else {
#if !(defined(LNS_KNOCK) && (LNS_KNOCK & 1))
#pragma unroll
                    for (int u = 0; u < NU; ++u) flush_unit(u, Xn);
#endif
                }
                // schedule: ALL LDS reads of the k-step first (next k-step's fragments + next pair's table entries:
                // nothing in this k-step consumes them), then after each MFMA a few of the step's other instructions
                __builtin_amdgcn_sched_group_barrier(0x100, 2 * SPL * (MT + NT) / 2 + 1, 0);
#pragma unroll
                for (int g = 0; g < (SPL == 3 ? 6 : 3) * MT * NT; ++g) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // MFMA
                    __builtin_amdgcn_sched_group_barrier(0x002, SPL == 3 ? 5 : 8, 0);   // VALU
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
    else if (pro_mode == 3) {                            // (f16x2 128-pixel tiles, 64 or 32 couts: the planner's rule)
        if constexpr (SPL == 2 && NTAP == 9 && !FUSE2 && NT == 1) k_loop(std::integral_constant<int, 3>{});
    }
    else if (pro_mode == 1) k_loop(std::integral_constant<int, 1>{});
    else k_loop(std::integral_constant<int, 0>{});

    // ---- epilogue (fp32) ---------------------------------------------------------
    int pix[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int p = (wn * NT + nt) * 32 + l31;
        int oy = ty * BH + (p >> a.bw_log2), ox = tx * BW + (p & (BW - 1));
        if (UP2) { oy = 2 * oy + pa; ox = 2 * ox + pb; }     // source pixel -> this phase's output pixel
        pix[nt] = (oy < a.Hout && ox < a.Wout) ? oy * a.Wout + ox : -1;
    }
    unsigned am = 0u;
    LNS_TSTAMP(3)
    convb_epilogue<NT, FUSE2, MT, true, true, false, false, (FUSE2 && LNS_NTS_CONV3F)>(a, acc_hi, acc_lo, pix, b, ct, kh, l31, tid, lds, xinv, am,
                                  (a.bias || a.badd) ? addv : nullptr, UP2 ? (ty * a.tiles_x + tx) * 4 + phase : -1 LNS_ETS_ARG,
                                  UP2 ? 4 : 1);
    LNS_TSTAMP(4)
    if (a.amax_out) amax_publish_block(a.amax_out, b, am, wmax);    // wmax: free since the prologue
    LNS_TS_DUMP
}

// ===========================================================================
// 1x1 convolution on the bf16 matrix pipe (same split scheme as the 3x3 kernel above).
//   tile  : 64 couts x 128 consecutive pixels of one sample, 4 waves (wave = 64 couts x 32 pixels)
//   stage : 32 input channels = 2 MFMA k-steps (K = 16 channels: lane half kh takes one 8-channel octet)
//   LDS   : pixels  [split][octet 0..3][pixel 0..127][8 ch] bf16, weights [split][octet][cout][8 ch] bf16
//   staging unit = (pixel, octet): 8 channel values of one pixel, two units per thread per stage
// A 1x1 conv has no tap reuse, so the fp32 -> 3 x bf16 split (VALU) is about as much work as the MFMAs;
// it is interleaved with them the same way as in the 3x3 kernel.
// ===========================================================================
// LDS slot of pixel p inside an octet row of the 1x1 kernels' pixel image [split][octet][pixel][8 ch]: adjacent pairs of
// slots are swapped in every other group of eight.  The staging threads own pixel PAIRS (8-byte global loads), so the eight
// lanes of a ds_write_b128 group are 32 bytes apart and, unswizzled, lanes i and i + 4 fall on the same four banks (write
// banking is (address / 4) mod 32): a two-way conflict on every patch write -- 24 - 30 % of the LDS-array cycles of these
// kernels in profiles/r03_pmc.json.  With the swap the eight lanes cover all 32 banks; the fragment reads (16 consecutive
// pixels per ds_read_b128 lane group, banking mod 64) stay conflict-free.  LNS_CONV1_NO_SWIZZLE: A/B build knob.
// (scale, shift) table of the prologue: only launches that have one pay for it (to_out's 512 channels: 4 KB -- the
// difference between two and three blocks per CU for the fused form)
__host__ __device__ inline int convb1_ss_floats(const ConvArgs& a) { return (a.ss != nullptr || a.gn_part != nullptr) ? a.Cin_pad * 2 : 0; }
__device__ __forceinline__ int conv1_slot(int p) {
#ifdef LNS_CONV1_NO_SWIZZLE
    return p;
#else
    return p ^ ((p >> 3) & 1);
#endif
}
// split scheme of the 1x1 kernels: 2 = two fp16 terms of the scaled operand (f16x2, see the 3x3 kernel), 3 = three bf16 terms
#define CONVB1_SPL 2
// 1: the three products of the f16x2 scheme go into ONE fp32 accumulator per tile (an fp32 chain's accuracy; 32 fewer
// registers -> three blocks per CU for these memory-bound kernels).  0: hh' and hl' + lh' in separate accumulators.
#ifndef LNS_CONV1_ONEACC
#define LNS_CONV1_ONEACC 1
#endif
#define CONVB1_ONEACC (LNS_CONV1_ONEACC != 0)
#define CONVB1_MIN_WAVES (LNS_CONV1_ONEACC ? 3 : 1)
#define CONVB1_SLAB_BYTES (CONVB1_SPL * 4 * 64 * 16)   // splits x 4 octets x 64 couts x 8 ch
template <bool VEC2, bool FUSE2>
// blocks per CU of the fused (1x1 + 1x1) form: a streaming kernel's HBM rate is its bytes in flight (one 16 KB stage per
// block) over the memory latency -- two blocks per CU measured 4.1 - 4.2 TB/s on FABlock to_out (512 -> 64 at 64^2)
#ifndef LNS_CONV1_FUSE2_WAVES
#define LNS_CONV1_FUSE2_WAVES 3
#endif
__global__ __launch_bounds__(256, FUSE2 ? (CONVB1_MIN_WAVES > LNS_CONV1_FUSE2_WAVES ? LNS_CONV1_FUSE2_WAVES : CONVB1_MIN_WAVES) : CONVB1_MIN_WAVES) void conv1_bf16x3_kernel(ConvArgs a) {
    constexpr int NTHR = 256, TM = 64, TN = 128, MT = 2, NT = 1, KC = 32, NJ = 2, NU = 2, SPL = CONVB1_SPL, NWU = CONVB1_SLAB_BYTES / 16 / 256;
    constexpr int XB = SPL * 4 * TN * 16;
    constexpr int BUF = XB + CONVB1_SLAB_BYTES;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* lds = smem;                                                  // 2 x [Xb | Wb]
    float* ssl = reinterpret_cast<float*>(lds + 2 * BUF);              // [Cin_pad][2]
    float* addv = ssl + convb1_ss_floats(a);                           // [TM] bias + per-sample add of this cout tile
    unsigned* wmax = reinterpret_cast<unsigned*>(addv + TM);           // [4] per-wave share of the activation bound

    const int tid = threadIdx.x, lane = tid & 63, wn = tid >> 6;
    const int l31 = lane & 31, kh = lane >> 5;
    const int b = blockIdx.y + a.b0;
    int bid = blockIdx.x;
    const int ct = bid % a.cout_tiles;
    const int tx = bid / a.cout_tiles;
    const int HW = a.Hin * a.Win;
    const int p0 = tx * TN;
    const float* xb = a.x + (long)b * a.x_bs;
    const bool has_ss = a.ss != nullptr || a.gn_part != nullptr;
    const int pro_mode = has_ss ? (a.act_in == ACT_SWISH ? 2 : 1) : 0;
    LNS_TS_DECL
    LNS_TSTAMP(0)

    // (ssl / addv / the activation bound are staged in k_loop behind the first stage's global loads, and the barrier
    //  that publishes them comes after: one memory latency before the first split instead of two)

    // two staging units (pixel, octet) per thread.  VEC2 (even H*W): two adjacent pixels of one octet, fetched
    // with 8-byte loads; otherwise one pixel, octets o and o + 2.
    // (the octet is wave-uniform: kept in an SGPR, so a load's channel offset is scalar arithmetic and the loads take
    //  the buffer form -- lane offset in one VGPR, channel offset in an SGPR, no 64-bit vector address arithmetic)
    int upx[NU], uoct[NU], udm[NU];
    float uok[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        upx[u] = VEC2 ? 2 * (tid & 63) + u : (tid & 127);
        uoct[u] = __builtin_amdgcn_readfirstlane(VEC2 ? (tid >> 6) : (tid >> 7) + 2 * u);
        const bool pvalid = p0 + upx[u] < HW;
        udm[u] = pvalid ? (p0 + upx[u]) * 4 : 0;           // byte offset inside a channel plane
        uok[u] = pvalid ? 1.0f : 0.0f;                     // times the activation scale once the bound is known
    }
    float xinv = 1.0f;
    const char* wslab = reinterpret_cast<const char*>(a.wb) + (long)ct * (a.Cin_pad / KC) * CONVB1_SLAB_BYTES;
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(xb), 0, a.Cin * HW * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(wslab), 0,
                                                                        (a.Cin_pad / KC) * CONVB1_SLAB_BYTES, 0x00020000);
    const int cin_m1 = a.Cin - 1, hw4 = HW * 4;
    const int aoff = (kh * TM + l31) * 16;                 // + (s*4 + 2j) * TM*16 + mt*32*16
    const int boff = (kh * TN + conv1_slot(wn * 32 + l31)) * 16;       // + (s*4 + 2j) * TN*16

    f32x16 acc_hi[MT][NT], acc_lo[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc_hi[mt][0][r] = 0.0f; acc_lo[mt][0][r] = 0.0f; }

    float pv[NU][8];
    unsigned hq[NU][4], mq[NU][4], lq[NU][4];
    float wq[NWU][4];

    // channel pair cp of both units: global -> registers
    auto load_pairs = [&](int cp, int c0) __attribute__((always_inline)) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            // (a channel past Cin reads the last channel: finite data that meets zero weights)
            if (VEC2) {
                const int c = c0 + uoct[0] * 8 + 2 * cp + e;           // uniform per wave
                // (flat 8-byte loads: the buffer form of this streaming read measured 7 % slower on the HBM-bound
                //  64 -> 64 layer at 128^2, 122 vs 114 us, although it needs one vector instruction less per load)
                const char* cb = reinterpret_cast<const char*>(xb) + (long)min(c, cin_m1) * hw4;     // scalar
#ifdef LNS_CONV1_NT_LOADS
                const f32x2 tv = __builtin_nontemporal_load(reinterpret_cast<const f32x2*>(cb + (unsigned)udm[0]));
                const float2 t = make_float2(tv[0], tv[1]);
#else
                const float2 t = *reinterpret_cast<const float2*>(cb + (unsigned)udm[0]);
#endif
                pv[0][2 * cp + e] = t.x; pv[1][2 * cp + e] = t.y;
            } else {
#pragma unroll
                for (int u = 0; u < NU; ++u) {
                    const int c = c0 + uoct[u] * 8 + 2 * cp + e;
                    pv[u][2 * cp + e] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(xr, udm[u], min(c, cin_m1) * hw4, 0));
                }
            }
        }
    };
    auto split_pair = [&](auto mode_tag, int u, int cp, int c0) __attribute__((always_inline)) {
        constexpr int MODE = decltype(mode_tag)::value;
        float t[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            float v = pv[u][2 * cp + e];
            if (MODE >= 1) {
                const float2 st = *reinterpret_cast<const float2*>(ssl + 2 * (c0 + uoct[u] * 8 + 2 * cp + e));
                v = v * st.x + st.y;
            }
            if (MODE == 2) v = swish_fast(v);
            t[e] = v * uok[u];
        }
        if (SPL == 3) split3_pair(t[0], t[1], hq[u][cp], mq[u][cp], lq[u][cp]);
        else split2_pair_f16(t[0], t[1], hq[u][cp], mq[u][cp]);
    };
    auto flush_unit = [&](int u, char* Xn) __attribute__((always_inline)) {
        char* dst = Xn + (uoct[u] * TN + conv1_slot(upx[u])) * 16;
        *reinterpret_cast<uint4*>(dst) = make_uint4(hq[u][0], hq[u][1], hq[u][2], hq[u][3]);
        *reinterpret_cast<uint4*>(dst + 4 * TN * 16) = make_uint4(mq[u][0], mq[u][1], mq[u][2], mq[u][3]);
        if (SPL == 3) *reinterpret_cast<uint4*>(dst + 8 * TN * 16) = make_uint4(lq[u][0], lq[u][1], lq[u][2], lq[u][3]);
    };
    auto load_w = [&](int i, int c0) __attribute__((always_inline)) {
        const u32x4 t = __builtin_amdgcn_raw_buffer_load_b128(wr, (tid + i * NTHR) * 16, (c0 >> 5) * CONVB1_SLAB_BYTES, 0);
        wq[i][0] = __uint_as_float(t[0]); wq[i][1] = __uint_as_float(t[1]); wq[i][2] = __uint_as_float(t[2]); wq[i][3] = __uint_as_float(t[3]);
    };
    auto write_w = [&](int i, char* Wn) __attribute__((always_inline)) {
        *reinterpret_cast<float4*>(Wn + (tid + i * NTHR) * 16) = make_float4(wq[i][0], wq[i][1], wq[i][2], wq[i][3]);
    };
    auto load_frags = [&](int j, const char* Xs, const char* Ws, uint4 (&af)[SPL][MT], uint4 (&bf)[SPL])
                          __attribute__((always_inline)) {
#pragma unroll
        for (int s = 0; s < SPL; ++s) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
                af[s][mt] = *reinterpret_cast<const uint4*>(Ws + (s * 4 + 2 * j) * (TM * 16) + mt * (32 * 16) + aoff);
            bf[s] = *reinterpret_cast<const uint4*>(Xs + (s * 4 + 2 * j) * (TN * 16) + boff);
        }
    };

    auto k_loop = [&](auto mode_tag) __attribute__((always_inline)) {
        const int last = a.Cin_pad - KC;
#pragma unroll
        for (int cp = 0; cp < 4; ++cp) load_pairs(cp, 0);
#pragma unroll
        for (int i = 0; i < NWU; ++i) load_w(i, 0);
        {
            float addreg = 0.0f;
            if (tid < TM) {
                const int co = ct * TM + tid, cc = co < a.Cout ? co : 0;
                addreg = (a.bias ? a.bias[cc] : 0.0f) + (a.badd ? a.badd[(long)b * a.Cout + cc] : 0.0f);
            }
            stage_ss_bound(a, b, ssl, wmax, tid, NTHR, has_ss);
            if (tid < TM) addv[tid] = addreg;
        }
        __syncthreads();                                   // ssl / addv / wmax visible
        LNS_TSTAMP(1)
        if (SPL == 2) {
            const float xs = f16x2_scale(block_bound(a, wmax), xinv);
#pragma unroll
            for (int u = 0; u < NU; ++u) uok[u] *= xs;
        }
#pragma unroll
        for (int u = 0; u < NU; ++u) {
#pragma unroll
            for (int cp = 0; cp < 4; ++cp) split_pair(mode_tag, u, cp, 0);
            flush_unit(u, lds);
        }
#pragma unroll
        for (int i = 0; i < NWU; ++i) write_w(i, lds + XB);
        {
            const int c1 = KC < last ? KC : last;
#pragma unroll
            for (int cp = 0; cp < 4; ++cp) load_pairs(cp, c1);
#pragma unroll
            for (int i = 0; i < NWU; ++i) load_w(i, c1);
        }
        __syncthreads();
        LNS_TSTAMP(2)
        int buf = 0;
        for (int c0 = 0; c0 < a.Cin_pad; c0 += KC) {
            const char* Xs = lds + buf * BUF;
            const char* Ws = Xs + XB;
            char* Xn = lds + (buf ^ 1) * BUF;
            char* Wn = Xn + XB;
            const int cw = c0 + KC < last ? c0 + KC : last;
            const int cl2 = c0 + 2 * KC < last ? c0 + 2 * KC : last;
            uint4 af[2][SPL][MT], bf[2][SPL];
            load_frags(0, Xs, Ws, af[0], bf[0]);
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                if (j + 1 < NJ) load_frags(j + 1, Xs, Ws, af[(j + 1) & 1], bf[(j + 1) & 1]);
                auto& A = af[j & 1];
                auto& Bq = bf[j & 1];
#define LNS_BX1(ACC, SA, SB)                                                                          \
    _Pragma("unroll") for (int mt = 0; mt < MT; ++mt)                                                 \
        ACC[mt][0] = SPL == 3 ? __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, A[SA][mt]),              \
                                    __builtin_bit_cast(bf16x8, Bq[SB]), ACC[mt][0], 0, 0, 0)                                  \
                              : __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, A[SA][mt]),                \
                                    __builtin_bit_cast(f16x8, Bq[SB]), ACC[mt][0], 0, 0, 0);
                if (SPL == 3) {
                    LNS_BX1(acc_lo, 1, 1)
                    LNS_BX1(acc_hi, 0, 0)
                    LNS_BX1(acc_lo, 0, SPL - 1)
                    LNS_BX1(acc_lo, SPL - 1, 0)
                    LNS_BX1(acc_lo, 0, 1)
                    LNS_BX1(acc_lo, 1, 0)
                } else if (CONVB1_ONEACC) {
                    LNS_BX1(acc_hi, 0, 0)
                    LNS_BX1(acc_hi, 0, 1)
                    LNS_BX1(acc_hi, 1, 0)
                } else {
                    LNS_BX1(acc_hi, 0, 0)
                    LNS_BX1(acc_lo, 0, 1)
                    LNS_BX1(acc_lo, 1, 0)
                }
#undef LNS_BX1
                // k-step j stages channel pairs 2j, 2j+1 of both units and half of the weight slots
#pragma unroll
                for (int cp = 2 * j; cp < 2 * j + 2; ++cp) {
#pragma unroll
                    for (int u = 0; u < NU; ++u) split_pair(mode_tag, u, cp, cw);
                    load_pairs(cp, cl2);
                }
                if (j == NJ - 1) {
#pragma unroll
                    for (int u = 0; u < NU; ++u) flush_unit(u, Xn);
                }
#pragma unroll
                for (int i = 2 * j; i < 2 * j + 2; ++i)
                    if (i < NWU) { write_w(i, Wn); load_w(i, cl2); }
#pragma unroll
                for (int g = 0; g < (SPL == 3 ? 6 : 3) * MT; ++g) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // MFMA
                    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);   // DS read
                    __builtin_amdgcn_sched_group_barrier(0x002, 12, 0);  // VALU
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

    int pix[NT];
    {
        const int p = p0 + wn * 32 + l31;
        pix[0] = p < a.Hout * a.Wout ? p : -1;
    }
    unsigned am = 0u;
    LNS_TSTAMP(3)
    convb_epilogue<NT, FUSE2, 2, true, true, false, false, (FUSE2 && LNS_NTS_CONV1F)>(a, acc_hi, acc_lo, pix, b, ct, kh, l31, tid, lds, xinv, am, (a.bias || a.badd) ? addv : nullptr, -1 LNS_ETS_ARG);
    LNS_TSTAMP(4)
    if (a.amax_out) amax_publish_block(a.amax_out, b, am, wmax);
    LNS_TS_DUMP
}

// Input-stationary form of the 1x1 kernel for narrow inputs (Cin_pad <= 64) feeding many output channels:
// the pixel tile is transformed, split and staged ONCE (it fits the two stage buffers), then the block walks
// over `a.ct_per_block` cout tiles streaming only weight slabs.  Same accumulation order per output as the
// streaming form (stage 0 then stage 1, k-steps in order), so either form gives the same bits.
// (three waves per SIMD although the 168-register budget spills 62 registers outside the loop: the in_proj shape runs
//  166 us that way and 195 us at two waves without spills)
template <bool VEC2>
__global__ __launch_bounds__(256, CONVB1_MIN_WAVES) void conv1s_bf16x3_kernel(ConvArgs a) {
    constexpr int NTHR = 256, TM = 64, TN = 128, MT = 2, NT = 1, KC = 32, NJ = 2, NU = 2, SPL = CONVB1_SPL, NWU = CONVB1_SLAB_BYTES / 16 / 256;
    constexpr int XB = SPL * 4 * TN * 16;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* xres = smem;                                                 // [stage 0..1][Xb]
    char* wbuf = smem + 2 * XB;                                        // [2][slab]
    float* ssl = reinterpret_cast<float*>(wbuf + 2 * CONVB1_SLAB_BYTES);
    unsigned* wmax = reinterpret_cast<unsigned*>(ssl + convb1_ss_floats(a));   // [4] per-wave share of the activation bound

    const int tid = threadIdx.x, lane = tid & 63, wn = tid >> 6;
    const int l31 = lane & 31, kh = lane >> 5;
    const int b = blockIdx.y + a.b0;
    const int nchunk = (a.cout_tiles + a.ct_per_block - 1) / a.ct_per_block;
    const int chunk = blockIdx.x % nchunk, tx = blockIdx.x / nchunk;
    const int ct0 = chunk * a.ct_per_block;
    const int nct = min(a.ct_per_block, a.cout_tiles - ct0);
    const int nstage = a.Cin_pad / KC;                                 // 1 or 2
    const int HW = a.Hin * a.Win;
    const int p0 = tx * TN;
    const float* xb = a.x + (long)b * a.x_bs;
    const bool has_ss = a.ss != nullptr || a.gn_part != nullptr;
    LNS_TS_DECL
    LNS_TSTAMP(0)

    float xinv = 1.0f;

    // ---- stage the whole pixel tile (all channels) ----------------------------------
    {
        int upx[NU], uoct[NU], udm[NU];
        float uok[NU];
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            upx[u] = VEC2 ? 2 * (tid & 63) + u : (tid & 127);
            uoct[u] = VEC2 ? (tid >> 6) : (tid >> 7) + 2 * u;
            const bool pvalid = p0 + upx[u] < HW;
            udm[u] = pvalid ? p0 + upx[u] : 0;
            uok[u] = pvalid ? 1.0f : 0.0f;
        }
        for (int st = 0; st < nstage; ++st) {
            float pv[NU][8];
#pragma unroll
            for (int ce = 0; ce < 8; ++ce) {
                if (VEC2) {
                    const int c = st * KC + uoct[0] * 8 + ce;
                    const float2 t = *reinterpret_cast<const float2*>(xb + (long)(c < a.Cin ? c : 0) * HW + udm[0]);
                    pv[0][ce] = t.x; pv[1][ce] = t.y;
                } else {
#pragma unroll
                    for (int u = 0; u < NU; ++u) {
                        const int c = st * KC + uoct[u] * 8 + ce;
                        pv[u][ce] = xb[(long)(c < a.Cin ? c : 0) * HW + udm[u]];
                    }
                }
            }
            if (st == 0) {
                stage_ss_bound(a, b, ssl, wmax, tid, NTHR, has_ss);  // behind the first stage's global loads
                __syncthreads();                            // ssl / wmax visible
                LNS_TSTAMP(1)
                if (SPL == 2) {
                    const float xs = f16x2_scale(block_bound(a, wmax), xinv);
#pragma unroll
                    for (int u = 0; u < NU; ++u) uok[u] *= xs;
                }
            }
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                unsigned hq[4], mq[4], lq[4];
#pragma unroll
                for (int cp = 0; cp < 4; ++cp) {
                    float t[2];
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        float v = pv[u][2 * cp + e];
                        if (has_ss) {
                            const float2 sv = *reinterpret_cast<const float2*>(ssl + 2 * (st * KC + uoct[u] * 8 + 2 * cp + e));
                            v = v * sv.x + sv.y;
                            if (a.act_in == ACT_SWISH) v = swish_fast(v);
                        }
                        t[e] = v * uok[u];
                    }
                    if (SPL == 3) split3_pair(t[0], t[1], hq[cp], mq[cp], lq[cp]);
                    else split2_pair_f16(t[0], t[1], hq[cp], mq[cp]);
                }
                char* dst = xres + st * XB + (uoct[u] * TN + conv1_slot(upx[u])) * 16;
                *reinterpret_cast<uint4*>(dst) = make_uint4(hq[0], hq[1], hq[2], hq[3]);
                *reinterpret_cast<uint4*>(dst + 4 * TN * 16) = make_uint4(mq[0], mq[1], mq[2], mq[3]);
                if (SPL == 3) *reinterpret_cast<uint4*>(dst + 8 * TN * 16) = make_uint4(lq[0], lq[1], lq[2], lq[3]);
            }
        }
    }

    // ---- walk over (cout tile, stage) pairs, streaming weight slabs ---------------------
    const int aoff = (kh * TM + l31) * 16;
    const int boff = (kh * TN + conv1_slot(wn * 32 + l31)) * 16;
    const int nit = nct * nstage;
    const char* wslab0 = reinterpret_cast<const char*>(a.wb) + (long)ct0 * nstage * CONVB1_SLAB_BYTES;   // slabs are (ct, stage)-major
    float wq[NWU][4];
    auto load_w = [&](int i, int it) __attribute__((always_inline)) {
        const int itc = it < nit ? it : nit - 1;
        const float4 t = *reinterpret_cast<const float4*>(wslab0 + (long)itc * CONVB1_SLAB_BYTES + (long)(tid + i * NTHR) * 16);
        wq[i][0] = t.x; wq[i][1] = t.y; wq[i][2] = t.z; wq[i][3] = t.w;
    };
    auto write_w = [&](int i, char* Wn) __attribute__((always_inline)) {
        *reinterpret_cast<float4*>(Wn + (long)(tid + i * NTHR) * 16) = make_float4(wq[i][0], wq[i][1], wq[i][2], wq[i][3]);
    };
#pragma unroll
    for (int i = 0; i < NWU; ++i) load_w(i, 0);
#pragma unroll
    for (int i = 0; i < NWU; ++i) write_w(i, wbuf);
#pragma unroll
    for (int i = 0; i < NWU; ++i) load_w(i, 1);
    __syncthreads();
    LNS_TSTAMP(2)

    f32x16 acc_hi[MT][NT], acc_lo[MT][NT];
    int pix[NT];
    {
        const int p = p0 + wn * 32 + l31;
        pix[0] = p < a.Hout * a.Wout ? p : -1;
    }
    int st = 0, ctl = 0;
    unsigned am = 0u;
    for (int it = 0; it < nit; ++it) {
        if (st == 0) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) { acc_hi[mt][0][r] = 0.0f; acc_lo[mt][0][r] = 0.0f; }
        }
        const char* Xs = xres + st * XB;
        const char* Ws = wbuf + (it & 1) * CONVB1_SLAB_BYTES;
        char* Wn = wbuf + ((it + 1) & 1) * CONVB1_SLAB_BYTES;
        uint4 af[2][SPL][MT], bf[2][SPL];
        auto load_frags = [&](int j, uint4 (&afj)[SPL][MT], uint4 (&bfj)[SPL]) __attribute__((always_inline)) {
#pragma unroll
            for (int s = 0; s < SPL; ++s) {
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
                    afj[s][mt] = *reinterpret_cast<const uint4*>(Ws + (s * 4 + 2 * j) * (TM * 16) + mt * (32 * 16) + aoff);
                bfj[s] = *reinterpret_cast<const uint4*>(Xs + (s * 4 + 2 * j) * (TN * 16) + boff);
            }
        };
        load_frags(0, af[0], bf[0]);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            if (j + 1 < NJ) load_frags(j + 1, af[(j + 1) & 1], bf[(j + 1) & 1]);
            auto& A = af[j & 1];
            auto& Bq = bf[j & 1];
#define LNS_BX1(ACC, SA, SB)                                                                          \
    _Pragma("unroll") for (int mt = 0; mt < MT; ++mt)                                                 \
        ACC[mt][0] = SPL == 3 ? __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, A[SA][mt]),              \
                                    __builtin_bit_cast(bf16x8, Bq[SB]), ACC[mt][0], 0, 0, 0)                                  \
                              : __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, A[SA][mt]),                \
                                    __builtin_bit_cast(f16x8, Bq[SB]), ACC[mt][0], 0, 0, 0);
            if (SPL == 3) {
                LNS_BX1(acc_lo, 1, 1)
                LNS_BX1(acc_hi, 0, 0)
                LNS_BX1(acc_lo, 0, SPL - 1)
                LNS_BX1(acc_lo, SPL - 1, 0)
                LNS_BX1(acc_lo, 0, 1)
                LNS_BX1(acc_lo, 1, 0)
            } else if (CONVB1_ONEACC) {
                LNS_BX1(acc_hi, 0, 0)
                LNS_BX1(acc_hi, 0, 1)
                LNS_BX1(acc_hi, 1, 0)
            } else {
                LNS_BX1(acc_hi, 0, 0)
                LNS_BX1(acc_lo, 0, 1)
                LNS_BX1(acc_lo, 1, 0)
            }
#undef LNS_BX1
#pragma unroll
            for (int i = 2 * j; i < 2 * j + 2; ++i)
                if (i < NWU) { write_w(i, Wn); load_w(i, it + 2); }
#pragma unroll
            for (int g = 0; g < (SPL == 3 ? 6 : 3) * MT; ++g) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
                __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();
        if (++st == nstage) {
            convb_epilogue<NT, false, MT, false, false>(a, acc_hi, acc_lo, pix, b, ct0 + ctl, kh, l31, tid, smem, xinv, am);
            st = 0;
            ++ctl;
        }
    }
    LNS_TSTAMP(3)
    LNS_TSTAMP(4)
    if (a.amax_out) amax_publish_block(a.amax_out, b, am, wmax);    // once per block, over all its cout tiles
    LNS_TS_DUMP
}

size_t convb1_lds_bytes(const ConvArgs& a) { return 2 * (CONVB1_SPL * 4 * 128 * 16 + CONVB1_SLAB_BYTES) + (size_t)convb1_ss_floats(a) * 4 + 64 * 4 + 16 + 16; }

bool convb1_fits(const ConvArgs& a) {
    return a.ks == 1 && a.stride == 1 && (a.Cin_pad % 32) == 0 && a.wb != nullptr && convb1_lds_bytes(a) <= 150 * 1024;
}

size_t convb1_weight_bytes(int Cout, int Cin_pad) { return (size_t)((Cout + 63) / 64) * (Cin_pad / 32) * CONVB1_SLAB_BYTES; }

// a split-operand launch without a bound on its input would have to guess the activation scale: refuse it
static bool has_act_bound(const ConvArgs& a) { return a.amax_in != nullptr || a.amax_in_const > 0.0f; }

hipError_t launch_conv1_bf16x3(const ConvArgs& a, hipStream_t s) {
    if (!convb1_fits(a)) return hipErrorInvalidValue;
    if (CONVB1_SPL == 2 && !has_act_bound(a)) return hipErrorInvalidValue;
    dim3 grid(a.tiles_x * a.cout_tiles, a.B);
    const size_t lds = convb1_lds_bytes(a);
    const bool vec2 = ((a.Hin * a.Win) % 2 == 0) && ((reinterpret_cast<uintptr_t>(a.x) & 7) == 0) && (a.x_bs % 2 == 0);
    if (a.ct_per_block > 0) {     // input-stationary form (planner: Cin_pad <= 64, several cout tiles, no fused conv)
        if (a.w2 || a.Cin_pad > 64) return hipErrorInvalidValue;
        const int nchunk = (a.cout_tiles + a.ct_per_block - 1) / a.ct_per_block;
        dim3 gs(a.tiles_x * nchunk, a.B);
        if (vec2) hipLaunchKernelGGL((conv1s_bf16x3_kernel<true>), gs, dim3(256), lds, s, a);
        else hipLaunchKernelGGL((conv1s_bf16x3_kernel<false>), gs, dim3(256), lds, s, a);
        return hipGetLastError();
    }
    if (a.w2) {
        if (vec2) hipLaunchKernelGGL((conv1_bf16x3_kernel<true, true>), grid, dim3(256), lds, s, a);
        else hipLaunchKernelGGL((conv1_bf16x3_kernel<false, true>), grid, dim3(256), lds, s, a);
    } else {
        if (vec2) hipLaunchKernelGGL((conv1_bf16x3_kernel<true, false>), grid, dim3(256), lds, s, a);
        else hipLaunchKernelGGL((conv1_bf16x3_kernel<false, false>), grid, dim3(256), lds, s, a);
    }
    return hipGetLastError();
}

size_t convb_lds_bytes(const ConvArgs& a, int tm, int spl, int ring) {
    const size_t pp1 = (size_t)a.PH * a.PW + 1;
    const size_t slab = a.up2 ? (size_t)spl * 4 * 64 * 16 : (size_t)CONVB_SLAB_BYTES * spl / 3 * tm / 64;
    // the epilogue reuses the stage buffers: GroupNorm tile statistics need 64 x 133 floats, the fused 1x1 conv its weights
    const size_t stage = std::max(ring * (spl * pp1 * 16 + slab), (size_t)64 * 133 * 4 + 64);
    return stage + spl * 16 + ((size_t)a.Cin_pad * 2 + 64) * 4 + 16 + 16;
}

bool convb_fits(const ConvArgs& a) {
    return a.ks == 3 && a.stride == 1 && (a.Cin_pad % 8) == 0 && a.wb != nullptr &&
           (long)a.PH * a.PW <= CONVB_MAXU * 256 && convb_lds_bytes(a, 64, 3, 2) <= 150 * 1024;
}

size_t convb_weight_bytes(int Cout, int Cin_pad) {
    return (size_t)((Cout + 63) / 64) * (Cin_pad / 8) * CONVB_SLAB_BYTES;     // the fp16 form needs 2/3 of it
}

// fp32 -> fp16 bits, round to nearest even, subnormals and overflow handled (host side of the f16x2 scheme)
static inline uint16_t host_f16_rne(float x, float* back) {
    uint32_t u;
    __builtin_memcpy(&u, &x, 4);
    const uint32_t sign = (u >> 16) & 0x8000u;
    const int32_t e = (int32_t)((u >> 23) & 0xff) - 127 + 15;
    uint32_t m = u & 0x7fffffu;
    uint16_t hbits;
    if (((u >> 23) & 0xff) == 0xff) hbits = (uint16_t)(sign | 0x7c00u | (m ? 0x200u : 0));
    else if (e >= 31) hbits = (uint16_t)(sign | 0x7c00u);
    else if (e <= 0) {
        if (e < -10) hbits = (uint16_t)sign;
        else {
            m |= 0x800000u;
            const int shift = 14 - e;                     // 14..24
            const uint32_t q = m >> shift, rem = m & ((1u << shift) - 1), halfway = 1u << (shift - 1);
            hbits = (uint16_t)(sign | (q + ((rem > halfway || (rem == halfway && (q & 1))) ? 1 : 0)));
        }
    } else {
        const uint32_t q = m >> 13, rem = m & 0x1fffu;
        uint32_t v = ((uint32_t)e << 10) | q;
        if (rem > 0x1000u || (rem == 0x1000u && (q & 1))) ++v;   // may carry into the exponent (correct)
        hbits = (uint16_t)(sign | v);
    }
    // back-conversion
    const uint32_t he = (hbits >> 10) & 0x1f, hm = hbits & 0x3ff;
    float f;
    if (he == 0) f = (float)hm * 5.9604644775390625e-8f;                       // 2^-24
    else if (he == 31) f = __builtin_inff();
    else { const uint32_t fu = ((he - 15 + 127) << 23) | (hm << 13); __builtin_memcpy(&f, &fu, 4); }
    *back = (hbits & 0x8000u) ? -f : f;
    return hbits;
}

// f16x2 slabs: [cout tile 64][stage of 8 ch][split 2][tap 9][64 cout][8 ch] fp16 of w * wscale (wscale: power of two)
void convf_pack_weight(void* dst, const float* w, int co0, int cout, int cin, int Cin_pad, float wscale) {
    uint16_t* d = static_cast<uint16_t*>(dst);
    const int nstage = Cin_pad / 8;
    for (int co = 0; co < cout; ++co) {
        const int cog = co0 + co, ct = cog / 64, cl = cog % 64;
        for (int ci = 0; ci < cin; ++ci) {
            const int st = ci / 8, c = ci % 8;
            for (int t = 0; t < 9; ++t) {
                const float v = w[((size_t)co * cin + ci) * 9 + t] * wscale;
                float hb, lb;
                uint16_t q[2];
                q[0] = host_f16_rne(v, &hb);
                q[1] = host_f16_rne(v - hb, &lb);
                for (int sidx = 0; sidx < 2; ++sidx) {
                    const size_t unit = (((size_t)ct * nstage + st) * 2 + sidx) * 9 + t;
                    d[(unit * 64 + cl) * 8 + c] = q[sidx];
                }
            }
        }
    }
}

// Phase slabs of the 2x-upsample form: [cout tile][stage][phase pa*2+pb][split 2][tap ty*2+tx][cout 64][8 ch] fp16; the taps
// of the 3x3 kernel that fall on the same source pixel are summed (in double) before the scale and the split.
size_t convu_weight_bytes(int Cout, int Cin_pad) { return (size_t)((Cout + 63) / 64) * (Cin_pad / 8) * 4 * (2 * 4 * 64 * 16); }
void convu_pack_weight(void* dst, const float* w, int co0, int cout, int cin, int Cin_pad, float wscale) {
    uint16_t* d = static_cast<uint16_t*>(dst);
    const int nstage = Cin_pad / 8;
    static const int lo[2][2] = {{0, 1}, {0, 2}}, hi[2][2] = {{0, 2}, {1, 2}};      // [phase bit][tap bit]: ky range
    for (int co = 0; co < cout; ++co) {
        const int cog = co0 + co, ct = cog / 64, cl = cog % 64;
        for (int ci = 0; ci < cin; ++ci) {
            const int st = ci / 8, c = ci % 8;
            const float* wk = w + ((size_t)co * cin + ci) * 9;
            for (int ph = 0; ph < 4; ++ph)
                for (int t = 0; t < 4; ++t) {
                    const int pa = ph >> 1, pb = ph & 1, ty = t >> 1, tx = t & 1;
                    double sum = 0.0;
                    for (int ky = lo[pa][ty]; ky <= hi[pa][ty]; ++ky)
                        for (int kx = lo[pb][tx]; kx <= hi[pb][tx]; ++kx) sum += (double)wk[ky * 3 + kx];
                    const float v = (float)sum * wscale;
                    float hb, lb;
                    uint16_t q[2];
                    q[0] = host_f16_rne(v, &hb);
                    q[1] = host_f16_rne(v - hb, &lb);
                    for (int sidx = 0; sidx < 2; ++sidx) {
                        const size_t unit = ((((size_t)ct * nstage + st) * 4 + ph) * 2 + sidx) * 4 + t;
                        d[(unit * 64 + cl) * 8 + c] = q[sidx];
                    }
                }
        }
    }
}

static inline uint16_t host_bf16_rne(float x, float* back) {
    uint32_t u;
    __builtin_memcpy(&u, &x, 4);
    u += 0x7fffu + ((u >> 16) & 1u);
    u &= 0xffff0000u;
    __builtin_memcpy(back, &u, 4);
    return (uint16_t)(u >> 16);
}

void convb_pack_weight(void* dst, const float* w, int co0, int cout, int cin, int Cin_pad) {
    uint16_t* d = static_cast<uint16_t*>(dst);
    const int nstage = Cin_pad / 8;
    for (int co = 0; co < cout; ++co) {
        const int cog = co0 + co, ct = cog / 64, cl = cog % 64;
        for (int ci = 0; ci < cin; ++ci) {
            const int st = ci / 8, c = ci % 8;
            for (int t = 0; t < 9; ++t) {
                const float v = w[((size_t)co * cin + ci) * 9 + t];
                float hb, mb, lb;
                uint16_t q[3];
                q[0] = host_bf16_rne(v, &hb);
                q[1] = host_bf16_rne(v - hb, &mb);
                q[2] = host_bf16_rne((v - hb) - mb, &lb);
                for (int sidx = 0; sidx < 3; ++sidx) {
                    const size_t unit = (((size_t)ct * nstage + st) * 3 + sidx) * 9 + t;
                    d[(unit * 64 + cl) * 8 + c] = q[sidx];
                }
            }
        }
    }
}

bool convb1_is_f16() { return CONVB1_SPL == 2; }

float convf_scale_for_bound(float bound) {
    uint32_t u;
    __builtin_memcpy(&u, &bound, 4);
    int f = 127 + CONVF_TARGET_EXP + 127 - (int)((u >> 23) & 0xffu);
    f = f < 17 ? 17 : (f > 247 ? 247 : f);
    const uint32_t sb = (uint32_t)f << 23;
    float sc;
    __builtin_memcpy(&sc, &sb, 4);
    return sc;
}

void convb1_pack_weight(void* dst, const float* w, int co0, int cout, int cin, int Cin_pad, float wscale) {
    if (CONVB1_SPL == 2) {
        uint16_t* d = static_cast<uint16_t*>(dst);
        const int nstage = Cin_pad / 32;
        for (int co = 0; co < cout; ++co) {
            const int cog = co0 + co, ct = cog / 64, cl = cog % 64;
            for (int ci = 0; ci < cin; ++ci) {
                const int st = ci / 32, oct = (ci % 32) / 8, c = ci % 8;
                const float v = w[(size_t)co * cin + ci] * wscale;
                float hb, lb;
                uint16_t q[2];
                q[0] = host_f16_rne(v, &hb);
                q[1] = host_f16_rne(v - hb, &lb);
                for (int sidx = 0; sidx < 2; ++sidx) {
                    const size_t unit = (((size_t)ct * nstage + st) * 2 + sidx) * 4 + oct;
                    d[(unit * 64 + cl) * 8 + c] = q[sidx];
                }
            }
        }
        return;
    }
    uint16_t* d = static_cast<uint16_t*>(dst);
    const int nstage = Cin_pad / 32;
    for (int co = 0; co < cout; ++co) {
        const int cog = co0 + co, ct = cog / 64, cl = cog % 64;
        for (int ci = 0; ci < cin; ++ci) {
            const int st = ci / 32, oct = (ci % 32) / 8, c = ci % 8;
            const float v = w[(size_t)co * cin + ci];
            float hb, mb, lb;
            uint16_t q[3];
            q[0] = host_bf16_rne(v, &hb);
            q[1] = host_bf16_rne(v - hb, &mb);
            q[2] = host_bf16_rne((v - hb) - mb, &lb);
            for (int sidx = 0; sidx < 3; ++sidx) {
                const size_t unit = (((size_t)ct * nstage + st) * 3 + sidx) * 4 + oct;
                d[(unit * 64 + cl) * 8 + c] = q[sidx];
            }
        }
    }
}

hipError_t launch_conv_up2r(const ConvArgs& a, hipStream_t s);
hipError_t launch_conv_up2q(const ConvArgs& a, hipStream_t s);
hipError_t launch_conv_w8(const ConvArgs& a, hipStream_t s);
bool convw8_fits(const ConvArgs& a);
hipError_t launch_conv_up2d(const ConvArgs& a, hipStream_t s);
hipError_t launch_conv_bf16x3(int variant, const ConvArgs& a, hipStream_t s) {
    if (!convb_fits(a)) return hipErrorInvalidValue;
    if (cv_is_f16x2_3x3(variant) && !has_act_bound(a)) return hipErrorInvalidValue;
    dim3 grid(a.tiles_x * a.tiles_y * a.cout_tiles, a.B);
    const bool two = (long)a.PH * a.PW > 256;            // patch units per thread
    if (variant == CV_F256) {                             // 256-pixel tiles, a wave owns 64 couts x 64 pixels
        if ((long)a.PH * a.PW > 512) return hipErrorInvalidValue;
        const size_t lds = convb_lds_bytes(a, 64, 2, 2);
        if (a.w2) hipLaunchKernelGGL((conv3_bf16x3_kernel<2, 2, true, 2, 2>), grid, dim3(256), lds, s, a);
        else hipLaunchKernelGGL((conv3_bf16x3_kernel<2, 2, false, 2, 2>), grid, dim3(256), lds, s, a);
        return hipGetLastError();
    }
    if (a.x_oct && (a.up2 >= 2 || a.w8 == 1)) return hipErrorInvalidValue;       // (these forms read planar tensors)
    if (variant == CV_F64 && a.up2 == 4) return launch_conv_up2d(a, s);     // both column phases per block (conv3_up2d.inc): the planner's form
    if (variant == CV_F64 && a.up2 == 3) return launch_conv_up2q(a, s);     // all four phases per block, two blocks per CU (conv3_up2q.inc)
    if (variant == CV_F64 && a.up2 == 2) return launch_conv_up2r(a, s);     // ... with the source patch resident in LDS (conv3_up2r.inc)
    // OCT8 tensors (ConvArgs::x_oct / y_oct): whole octets, 32-bit byte offsets
    if ((a.x_oct && ((a.Cin & 7) || (long)a.Cin * a.Hin * a.Win * 4 >= (1L << 31) || !cv_is_f16x2_3x3(variant) || variant == CV_F256)) ||
        (a.y_oct && ((a.Cout & 7) || (long)a.Cout * a.Hout * a.Wout * 4 >= (1L << 31))))
        return hipErrorInvalidValue;
#define LNS_LAUNCH_F16X2(NU_, FUSE_, MT_, NTAP_, GRID)                                                                    \
    do {                                                                                                                  \
        if (a.x_oct) hipLaunchKernelGGL((conv3_bf16x3_kernel<1, NU_, FUSE_, MT_, 2, NTAP_, true>), GRID, dim3(256), lds, s, a);  \
        else hipLaunchKernelGGL((conv3_bf16x3_kernel<1, NU_, FUSE_, MT_, 2, NTAP_, false>), GRID, dim3(256), lds, s, a);  \
    } while (0)
    if (variant == CV_F64 && a.up2) {                     // phase-decomposed 2x nearest upsample + 3x3 (four taps per phase)
        const size_t lds = convb_lds_bytes(a, 64, 2, 2);
        dim3 gu(a.tiles_x * a.tiles_y * a.cout_tiles * 4, a.B);
        if (a.w2) {
            if (two) LNS_LAUNCH_F16X2(2, true, 2, 4, gu);
            else LNS_LAUNCH_F16X2(1, true, 2, 4, gu);
        } else {
            if (two) LNS_LAUNCH_F16X2(2, false, 2, 4, gu);
            else LNS_LAUNCH_F16X2(1, false, 2, 4, gu);
        }
        return hipGetLastError();
    }
    if (a.up2) return hipErrorInvalidValue;
    if (variant == CV_F64 && !a.w2 && a.w8 >= 0) {        // small launches: the 8-wave form (conv3_w8.inc) -- measured no faster,
        const long w8_below = knobs().conv_w8_below;      // so opt-in only (default 0)
        const long blocks = (long)a.tiles_x * a.tiles_y * a.cout_tiles * a.B;
        if ((a.w8 == 1 || blocks < w8_below) && convw8_fits(a)) return launch_conv_w8(a, s);
        if (a.w8 == 1) return hipErrorInvalidValue;
    }
    if (variant == CV_F64) {                              // two-term fp16 split
        const size_t lds = convb_lds_bytes(a, 64, 2, 2);
        if (a.w2) {
            if (two) LNS_LAUNCH_F16X2(2, true, 2, 9, grid);
            else LNS_LAUNCH_F16X2(1, true, 2, 9, grid);
        } else {
            if (two) LNS_LAUNCH_F16X2(2, false, 2, 9, grid);
            else LNS_LAUNCH_F16X2(1, false, 2, 9, grid);
        }
        return hipGetLastError();
    }
    if (variant == CV_F32) {                              // f16x2, 32-cout tiles: a.cout_tiles counts those
        if (a.w2) return hipErrorInvalidValue;
        const size_t lds = convb_lds_bytes(a, 32, 2, 2);
        if (two) LNS_LAUNCH_F16X2(2, false, 1, 9, grid);
        else LNS_LAUNCH_F16X2(1, false, 1, 9, grid);
        return hipGetLastError();
    }
#undef LNS_LAUNCH_F16X2
    if (variant == CV_B32) {                              // 32-cout tiles: a.cout_tiles counts those
        if (a.w2) return hipErrorInvalidValue;
        const size_t lds = convb_lds_bytes(a, 32, 3, 2);
        if (two) hipLaunchKernelGGL((conv3_bf16x3_kernel<1, 2, false, 1>), grid, dim3(256), lds, s, a);
        else hipLaunchKernelGGL((conv3_bf16x3_kernel<1, 1, false, 1>), grid, dim3(256), lds, s, a);
        return hipGetLastError();
    }
    const size_t lds = convb_lds_bytes(a, 64, 3, 2);
    if (a.w2) {
        if (two) hipLaunchKernelGGL((conv3_bf16x3_kernel<1, 2, true>), grid, dim3(256), lds, s, a);
        else hipLaunchKernelGGL((conv3_bf16x3_kernel<1, 1, true>), grid, dim3(256), lds, s, a);
    } else {
        if (two) hipLaunchKernelGGL((conv3_bf16x3_kernel<1, 2, false>), grid, dim3(256), lds, s, a);
        else hipLaunchKernelGGL((conv3_bf16x3_kernel<1, 1, false>), grid, dim3(256), lds, s, a);
    }
    return hipGetLastError();
}

// The dual-phase form of the upsampling conv: one block per (source tile, row phase), both column phases (ConvArgs::up2 == 4)
#include "conv3_up2d.inc"

// Four kernel forms that were built, proven bit-identical to the shipped kernels and MEASURED SLOWER or neutral (DESIGN.md
// sections 6d, 6e): producer / consumer waves (conv3_pc.inc), the resident-weights upsampling conv (conv3_up2r.inc), the 8-wave
// small-launch form (conv3_w8.inc), the quad-phase upsampling conv (conv3_up2q.inc, round 4: -7 % on the plain 64 -> 64 layer,
// +3 % on the one the decoder actually runs, the fused 3x3 + 1x1).  They are kept as source with their parity tests but only
// compiled with -DLNS_EXPERIMENTAL (make DIAGFLAGS=-DLNS_EXPERIMENTAL); the shipped library carries only kernels the planner uses.
#ifdef LNS_EXPERIMENTAL
#include "conv3_pc.inc"
#include "conv3_up2r.inc"
#include "conv3_up2q.inc"
#include "conv3_w8.inc"
bool build_has_experimental() { return true; }
#else
bool build_has_experimental() { return false; }
size_t convuq_lds_bytes(const ConvArgs&) { return 0; }
bool convuq_fits(const ConvArgs&) { return false; }
hipError_t launch_conv_up2q(const ConvArgs&, hipStream_t) { return hipErrorInvalidValue; }
size_t convpc_lds_bytes(const ConvArgs&, int) { return 0; }
bool convpc_geom_fits(const ConvArgs&, int) { return false; }
bool convpc_fits(const ConvArgs&, int) { return false; }
hipError_t launch_conv_pc(int, const ConvArgs&, hipStream_t) { return hipErrorInvalidValue; }
bool convur_fits(const ConvArgs&) { return false; }
size_t convur_lds_bytes(const ConvArgs&) { return 0; }
hipError_t launch_conv_up2r(const ConvArgs&, hipStream_t) { return hipErrorInvalidValue; }
bool convw8_fits(const ConvArgs&) { return false; }
hipError_t launch_conv_w8(const ConvArgs&, hipStream_t) { return hipErrorInvalidValue; }
#endif

// ===========================================================================
// Thin 1x1 projection (<= 4 output channels, e.g. the decoder's last 64 -> 3 conv): pure streaming, no matrix pipe.
// A thread owns 4 consecutive pixels and walks the input channels with 16-byte loads (8 in flight), applying the
// GroupNorm scale/shift + Swish prologue and accumulating the <= 4 outputs with fp32 FMAs in channel order.
// HBM-bound: one read of the input.
// ===========================================================================
__global__ __launch_bounds__(256) void conv1_thin_kernel(ConvArgs a) {
    __shared__ float wsm[4 * 512];          // [co][c]
    __shared__ float2 ssm[512];             // (scale, shift) per channel
    const int tid = threadIdx.x, b = blockIdx.y + a.b0;
    const int HW = a.Hin * a.Win, C = a.Cin, CO = a.Cout;
    const bool has_ss = a.ss != nullptr;
    for (int i = tid; i < CO * C; i += 256) {                     // fp32 pack [tap 1][Cin_pad][Cout_pad]
        const int co = i / C, c = i - co * C;
        wsm[co * 512 + c] = a.w[(long)c * a.Cout_pad + co];
    }
    for (int i = tid; i < C; i += 256)
        ssm[i] = has_ss ? make_float2(a.ss[((long)b * C + i) * 2], a.ss[((long)b * C + i) * 2 + 1]) : make_float2(1.0f, 0.0f);
    __syncthreads();
    const int p4r = blockIdx.x * 256 + tid;                       // group of 4 pixels
    const bool live = p4r * 4 < HW;                               // (a thread past the plane redoes group 0 and stores nothing)
    const int p4 = live ? p4r : 0;
    const float* xb = a.x + (long)b * a.x_bs + (long)p4 * 4;
    const bool swish = has_ss && a.act_in == ACT_SWISH;
    float acc[4][4];
#pragma unroll
    for (int co = 0; co < 4; ++co)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[co][e] = 0.0f;
    // (issuing the next 8 channels' loads before the current 8 are consumed measured no faster: 65.9 vs 65.7 us)
    for (int c0 = 0; c0 < C; c0 += 8) {
        float4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int c = c0 + u < C ? c0 + u : C - 1;
            // (a read-once stream: non-temporal loads measured 63.2 -> 56.9 us per launch on the decoder's 128^2 projection; the
            //  same on the streaming 1x1 kernel's input measured SLOWER, 66.2 -> 76.7 ms per 5 rollouts: LNS_CONV1_NT_LOADS)
            typedef float f32x4_t __attribute__((ext_vector_type(4)));
            const f32x4_t tv = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(xb + (long)c * HW));
            v[u] = make_float4(tv[0], tv[1], tv[2], tv[3]);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (c0 + u < C) {
                const float2 st = ssm[c0 + u];
                float t[4] = {v[u].x * st.x + st.y, v[u].y * st.x + st.y, v[u].z * st.x + st.y, v[u].w * st.x + st.y};
                if (swish) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) t[e] = swish_fast(t[e]);
                }
#pragma unroll
                for (int co = 0; co < 4; ++co) {
                    if (co < CO) {
                        const float wv = wsm[co * 512 + c0 + u];
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[co][e] = fmaf(wv, t[e], acc[co][e]);
                    }
                }
            }
        }
    }
    float* yb = y_base(a, b) + (long)p4 * 4;
    float bv[4];                                               // bias loads ahead of the stores
#pragma unroll
    for (int co = 0; co < 4; ++co) bv[co] = a.bias ? a.bias[co < CO ? co : 0] : 0.0f;
    unsigned am = 0u;
#pragma unroll
    for (int co = 0; co < 4; ++co) {
        if (co < CO && live) {
            const float4 o = make_float4(acc[co][0] + bv[co], acc[co][1] + bv[co], acc[co][2] + bv[co], acc[co][3] + bv[co]);
            *reinterpret_cast<float4*>(yb + (long)co * HW) = o;
            am = max(max(am, abs_bits(o.x)), max(max(abs_bits(o.y), abs_bits(o.z)), abs_bits(o.w)));
        }
    }
    if (a.amax_out) {                                          // uniform; one atomic per wave (16 blocks x 4 per 128^2 sample)
        const unsigned m = wave_umax(am);
        if ((tid & 63) == 0 && m) atomicMax(a.amax_out + (long)b * LNS_AMAX_SUB + ((blockIdx.x * 4 + (tid >> 6)) & (LNS_AMAX_SUB - 1)), m);
    }
}

bool conv1_thin_fits(const ConvArgs& a) {
    return a.ks == 1 && a.stride == 1 && a.Cout <= 4 && a.Cin <= 512 && ((a.Hin * a.Win) % 4) == 0 && !a.res && !a.badd &&
           a.act_out == ACT_NONE && !a.w2 && (a.act_in == ACT_NONE || a.act_in == ACT_SWISH) && (a.x_bs % 4) == 0 &&
           (a.y_bs % 4) == 0 && (a.y_bs2 % 4) == 0 && ((reinterpret_cast<uintptr_t>(a.x) | reinterpret_cast<uintptr_t>(a.y)) & 15) == 0;
}

hipError_t launch_conv1_thin(const ConvArgs& a, hipStream_t s) {
    if (!conv1_thin_fits(a)) return hipErrorInvalidValue;
    const int groups = a.Hin * a.Win / 4;
    hipLaunchKernelGGL(conv1_thin_kernel, dim3((groups + 255) / 256, a.B), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ===========================================================================
// GroupNorm statistics: one block per (group, sample); two-pass (mean, then
// centred second moment) over a contiguous (C/groups)*HW slab.  HBM-bound.
// ===========================================================================
// NV: float4 per thread held in registers by the single-read path (0: streaming two-read path only); small NV keeps
// the register count -- and with it the number of resident blocks -- right for small slabs
template <int NVT>
__global__ __launch_bounds__(256) void gn_stats_kernel(GnStatsArgs a) {
    __shared__ float red[4];
    const int g = blockIdx.x, b = blockIdx.y;
    const int cg = a.C / a.groups;
    const long n = (long)cg * a.HW;
    const float* xs = a.x + (long)b * a.x_bs + (long)g * cg * a.HW;
    const float* pm = a.premul ? a.premul + (long)b * a.C + g * cg : nullptr;
    float s = 0.0f, q = 0.0f;
    float mean;
    const bool vec = !pm && (n & 3) == 0 && ((reinterpret_cast<uintptr_t>(xs) & 15) == 0);
    constexpr int NV = NVT > 0 ? NVT : 1;
    if (NVT > 0 && vec && (n >> 2) <= (long)NV * 256) {
        // the whole slab fits the block's registers: ONE read (all loads in flight), exact two-pass statistics,
        // the same per-thread element order and reduction tree as the streaming path below
        const float4* x4 = reinterpret_cast<const float4*>(xs);
        const int n4 = (int)(n >> 2);
        float4 v[NV];
#pragma unroll
        for (int u = 0; u < NV; ++u) {
            const int i = threadIdx.x + u * 256;
            v[u] = i < n4 ? x4[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
#pragma unroll
        for (int u = 0; u < NV; ++u)
            if (threadIdx.x + u * 256 < n4) s += (v[u].x + v[u].y) + (v[u].z + v[u].w);
        mean = block_sum_256(s, red) / (float)n;
#pragma unroll
        for (int u = 0; u < NV; ++u)
            if (threadIdx.x + u * 256 < n4) {
                const float d0 = v[u].x - mean, d1 = v[u].y - mean, d2 = v[u].z - mean, d3 = v[u].w - mean;
                q += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
            }
    } else {
        if (vec) {
            const float4* x4 = reinterpret_cast<const float4*>(xs);
            const long n4 = n >> 2;
            for (long base = 0; base < n4; base += 256 * 8) {       // 8 loads in flight per thread
                float4 v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const long i = base + threadIdx.x + u * 256;
                    v[u] = i < n4 ? x4[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                }
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (base + threadIdx.x + u * 256 < n4) s += (v[u].x + v[u].y) + (v[u].z + v[u].w);
            }
        } else {
            for (long i = threadIdx.x; i < n; i += 256) {
                float v = xs[i];
                if (pm) v *= pm[i / a.HW];
                s += v;
            }
        }
        mean = block_sum_256(s, red) / (float)n;
        if (vec) {
            const float4* x4 = reinterpret_cast<const float4*>(xs);
            const long n4 = n >> 2;
            for (long base = 0; base < n4; base += 256 * 8) {
                float4 v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const long i = base + threadIdx.x + u * 256;
                    v[u] = i < n4 ? x4[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                }
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (base + threadIdx.x + u * 256 < n4) {
                        const float d0 = v[u].x - mean, d1 = v[u].y - mean, d2 = v[u].z - mean, d3 = v[u].w - mean;
                        q += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
                    }
            }
        } else {
            for (long i = threadIdx.x; i < n; i += 256) {
                float v = xs[i];
                if (pm) v *= pm[i / a.HW];
                const float d = v - mean;
                q += d * d;
            }
        }
    }
    const float var = block_sum_256(q, red) / (float)n;
    const float rstd = 1.0f / sqrtf(var + a.eps);
    for (int c = threadIdx.x; c < cg; c += 256) {
        const int ch = g * cg + c;
        const float ga = a.gamma ? a.gamma[ch] : 1.0f;
        const float be = a.beta ? a.beta[ch] : 0.0f;
        const float p = pm ? pm[c] : 1.0f;
        a.ss[((long)b * a.C + ch) * 2] = rstd * ga * p;
        a.ss[((long)b * a.C + ch) * 2 + 1] = be - mean * rstd * ga;
    }
}

// Two-stage variant for launches with few (sample, group) pairs (GroupNorm(1, C)): stage 1 gives
// every (sample, channel) plane its own block (mean and centred second moment), stage 2 merges
// the channels of a group with the pairwise update of Chan et al. -- exact two-pass numerics per
// plane, parallelism B*C instead of B*groups.
// Small groups (slab <= 4 KB, e.g. GroupNorm(32, 128) on a 16x16 latent): one WAVE per (group, sample), the slab in
// 4 float4 per lane, wave shuffles only -- no block barrier, 4 groups per 256-thread block.
__global__ __launch_bounds__(256) void gn_stats_wave_kernel(GnStatsArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = blockIdx.x * 4 + wave, b = blockIdx.y;
    if (g >= a.groups) return;
    const int cg = a.C / a.groups;
    const int n = cg * a.HW, n4 = n >> 2;
    const float4* x4 = reinterpret_cast<const float4*>(a.x + (long)b * a.x_bs + (long)g * cg * a.HW);
    float4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i = lane + u * 64;
        v[u] = i < n4 ? x4[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    float s = 0.0f;
#pragma unroll
    for (int u = 0; u < 4; ++u)
        if (lane + u * 64 < n4) s += (v[u].x + v[u].y) + (v[u].z + v[u].w);
    const float mean = wave_sum(s) / (float)n;
    float q = 0.0f;
#pragma unroll
    for (int u = 0; u < 4; ++u)
        if (lane + u * 64 < n4) {
            const float d0 = v[u].x - mean, d1 = v[u].y - mean, d2 = v[u].z - mean, d3 = v[u].w - mean;
            q += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
        }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)n + a.eps);
    for (int c = lane; c < cg; c += 64) {
        const int ch = g * cg + c;
        const float ga = a.gamma ? a.gamma[ch] : 1.0f;
        const float be = a.beta ? a.beta[ch] : 0.0f;
        a.ss[((long)b * a.C + ch) * 2] = rstd * ga;
        a.ss[((long)b * a.C + ch) * 2 + 1] = be - mean * rstd * ga;
    }
}

__global__ __launch_bounds__(256) void gn_partial_kernel(GnStatsArgs a, float* part) {
    __shared__ float red[4];
    const int c = blockIdx.x, b = blockIdx.y;
    const float* xs = a.x + (long)b * a.x_bs + (long)c * a.HW;
    const int n = a.HW;
    const bool v4 = (n & 3) == 0 && ((reinterpret_cast<uintptr_t>(xs) & 15) == 0);
    float s = 0.0f;
    if (v4) {
        const float4* x4 = reinterpret_cast<const float4*>(xs);
        for (int i = threadIdx.x; i < (n >> 2); i += 256) { const float4 v = x4[i]; s += (v.x + v.y) + (v.z + v.w); }
    } else {
        for (int i = threadIdx.x; i < n; i += 256) s += xs[i];
    }
    const float mean = block_sum_256(s, red) / (float)n;
    float q = 0.0f;
    if (v4) {
        const float4* x4 = reinterpret_cast<const float4*>(xs);
        for (int i = threadIdx.x; i < (n >> 2); i += 256) {
            const float4 v = x4[i];
            const float d0 = v.x - mean, d1 = v.y - mean, d2 = v.z - mean, d3 = v.w - mean;
            q += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
        }
    } else {
        for (int i = threadIdx.x; i < n; i += 256) { const float d = xs[i] - mean; q += d * d; }
    }
    const float m2 = block_sum_256(q, red);
    if (threadIdx.x == 0) { part[((long)b * a.C + c) * 2] = mean; part[((long)b * a.C + c) * 2 + 1] = m2; }
}

__global__ __launch_bounds__(64) void gn_finalize_kernel(GnStatsArgs a, const float* part) {
    const int g = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    const int cg = a.C / a.groups;
    const float* pm = a.premul ? a.premul + (long)b * a.C + g * cg : nullptr;
    const float n = (float)a.HW;
    // statistics of x * premul: mean_c -> p mean_c, M2_c -> p^2 M2_c
    float sm = 0.0f;
    for (int c = lane; c < cg; c += 64) {
        const float p = pm ? pm[c] : 1.0f;
        sm += p * part[((long)b * a.C + g * cg + c) * 2];
    }
    const float mean = wave_sum(sm) / (float)cg;
    float m2 = 0.0f;
    for (int c = lane; c < cg; c += 64) {
        const float p = pm ? pm[c] : 1.0f;
        const float mc = p * part[((long)b * a.C + g * cg + c) * 2];
        const float d = mc - mean;
        m2 += p * p * part[((long)b * a.C + g * cg + c) * 2 + 1] + n * d * d;
    }
    const float var = wave_sum(m2) / (n * (float)cg);
    const float rstd = 1.0f / sqrtf(var + a.eps);
    for (int c = lane; c < cg; c += 64) {
        const int ch = g * cg + c;
        const float ga = a.gamma ? a.gamma[ch] : 1.0f;
        const float be = a.beta ? a.beta[ch] : 0.0f;
        const float p = pm ? pm[c] : 1.0f;
        a.ss[((long)b * a.C + ch) * 2] = rstd * ga * p;
        a.ss[((long)b * a.C + ch) * 2 + 1] = be - mean * rstd * ga;
    }
}

// GroupNorm scale/shift from the per-tile (mean, M2) partials a convolution epilogue left: [B][tiles][C][2], every
// partial over GN_TILE_PIXELS values.  One block per (group, sample); fixed order, exact merge of equal-count sets.
// `count` pixels behind every partial (GN_TILE_PIXELS, or the plane of a ragged single tile); a.premul as in gn_stats_kernel.
__device__ __forceinline__ float gn_tile_count(const GnTileGeom& q, int t) {
    if (q.flat) return (float)min(GN_TILE_PIXELS, q.H * q.W - t * GN_TILE_PIXELS);
    const int BW = 1 << q.bw_log2, BH = GN_TILE_PIXELS >> q.bw_log2, ty = t / q.tiles_x, tx = t - ty * q.tiles_x;
    return (float)(min(BH, q.H - ty * BH) * min(BW, q.W - tx * BW));
}
// ragged tiling: partials over unequal pixel counts (fixed order; Chan et al. with weights)
__global__ __launch_bounds__(256) void gn_tile_finalize_ragged_kernel(GnStatsArgs a, const float* part, int tiles, GnTileGeom q) {
    __shared__ float red[4];
    const int g = blockIdx.x, b = blockIdx.y;
    const int cg = a.C / a.groups;
    const int E = tiles * cg;
    const float* pb = part + (long)b * tiles * a.C * 2;
    const float* pm = a.premul ? a.premul + (long)b * a.C + g * cg : nullptr;
    const float N = (float)cg * (float)(q.H * q.W);
    float sm = 0.0f;
    for (int i = threadIdx.x; i < E; i += 256) {
        const int t = i / cg, c = i - t * cg;
        const float mc = pb[((long)t * a.C + g * cg + c) * 2];
        sm += gn_tile_count(q, t) * (pm ? pm[c] * mc : mc);
    }
    const float mean = block_sum_256(sm, red) / N;
    float m2 = 0.0f;
    for (int i = threadIdx.x; i < E; i += 256) {
        const int t = i / cg, c = i - t * cg;
        const float* pp = pb + ((long)t * a.C + g * cg + c) * 2;
        const float n = gn_tile_count(q, t), p = pm ? pm[c] : 1.0f, d = p * pp[0] - mean;
        m2 += p * p * pp[1] + n * d * d;
    }
    const float var = block_sum_256(m2, red) / N;
    const float rstd = 1.0f / sqrtf(var + a.eps);
    for (int c = threadIdx.x; c < cg; c += 256) {
        const int ch = g * cg + c;
        const float ga = a.gamma ? a.gamma[ch] : 1.0f;
        const float be = a.beta ? a.beta[ch] : 0.0f;
        a.ss[((long)b * a.C + ch) * 2] = pm ? rstd * ga * pm[c] : rstd * ga;
        a.ss[((long)b * a.C + ch) * 2 + 1] = be - mean * rstd * ga;
    }
}

__global__ __launch_bounds__(256) void gn_tile_finalize_kernel(GnStatsArgs a, const float* part, int tiles, int count) {
    __shared__ float red[4];
    const int g = blockIdx.x, b = blockIdx.y;
    const int cg = a.C / a.groups;
    const int E = tiles * cg;
    const float* pb = part + (long)b * tiles * a.C * 2;
    const float* pm = a.premul ? a.premul + (long)b * a.C + g * cg : nullptr;
    const float cnt = (float)count;
    float sm = 0.0f;
    for (int i = threadIdx.x; i < E; i += 256) {
        const int t = i / cg, c = i - t * cg;
        const float mc = pb[((long)t * a.C + g * cg + c) * 2];
        sm += pm ? pm[c] * mc : mc;
    }
    const float mean = block_sum_256(sm, red) / (float)E;
    float m2 = 0.0f;
    for (int i = threadIdx.x; i < E; i += 256) {
        const int t = i / cg, c = i - t * cg;
        const float* pp = pb + ((long)t * a.C + g * cg + c) * 2;
        if (pm) { const float p = pm[c], d = p * pp[0] - mean; m2 += p * p * pp[1] + cnt * d * d; }
        else { const float d = pp[0] - mean; m2 += pp[1] + cnt * d * d; }
    }
    const float var = block_sum_256(m2, red) / (cnt * (float)E);
    const float rstd = 1.0f / sqrtf(var + a.eps);
    for (int c = threadIdx.x; c < cg; c += 256) {
        const int ch = g * cg + c;
        const float ga = a.gamma ? a.gamma[ch] : 1.0f;
        const float be = a.beta ? a.beta[ch] : 0.0f;
        a.ss[((long)b * a.C + ch) * 2] = pm ? rstd * ga * pm[c] : rstd * ga;
        a.ss[((long)b * a.C + ch) * 2 + 1] = be - mean * rstd * ga;
    }
}

hipError_t launch_gn_tile_finalize(const GnStatsArgs& a, const float* tile_part, int tiles, int count, GnTileGeom geom, hipStream_t s) {
    if (count > 0) hipLaunchKernelGGL(gn_tile_finalize_kernel, dim3(a.groups, a.B), dim3(256), 0, s, a, tile_part, tiles, count);
    else hipLaunchKernelGGL(gn_tile_finalize_ragged_kernel, dim3(a.groups, a.B), dim3(256), 0, s, a, tile_part, tiles, geom);
    return hipGetLastError();
}

bool gn_stats_two_stage(const GnStatsArgs& a) {
    // depends on the layer only, never on the batch: results stay bit-identical across batch sizes.
    // Wide groups go through per-channel partials + a merge, unless the whole group slab fits the registers of one
    // block (<= 128 KB, no per-channel pre-multiplier): then the single-read path of gn_stats_kernel is one launch.
    if (a.C / a.groups < 32) return false;
    const long n = (long)(a.C / a.groups) * a.HW;
    const bool in_regs = !a.premul && (n & 3) == 0 && (n >> 2) <= 32 * 256 && (a.x_bs & 3) == 0;
    return !in_regs;
}

hipError_t launch_gn_stats(const GnStatsArgs& a, float* part, hipStream_t s) {
    if (part && gn_stats_two_stage(a)) {
        hipLaunchKernelGGL(gn_partial_kernel, dim3(a.C, a.B), dim3(256), 0, s, a, part);
        hipLaunchKernelGGL(gn_finalize_kernel, dim3(a.groups, a.B), dim3(64), 0, s, a, static_cast<const float*>(part));
    } else {
        const long n = (long)(a.C / a.groups) * a.HW;
        const long per = ((n >> 2) + 255) / 256;            // float4 per thread if the slab is held in registers
        dim3 grid(a.groups, a.B);
        const bool al16 = (a.x_bs & 3) == 0 && ((a.HW * (a.C / a.groups)) & 3) == 0 && (reinterpret_cast<uintptr_t>(a.x) & 15) == 0;
        if (!(n & 3) && !a.premul && n <= 1024 && al16)     // layer-static choice (pointers are 256-byte aligned arena slots)
            hipLaunchKernelGGL(gn_stats_wave_kernel, dim3((a.groups + 3) / 4, a.B), dim3(256), 0, s, a);
        else if ((n & 3) || a.premul || per > 32) hipLaunchKernelGGL((gn_stats_kernel<0>), grid, dim3(256), 0, s, a);
        else if (per <= 1) hipLaunchKernelGGL((gn_stats_kernel<1>), grid, dim3(256), 0, s, a);
        else if (per <= 4) hipLaunchKernelGGL((gn_stats_kernel<4>), grid, dim3(256), 0, s, a);
        else if (per <= 8) hipLaunchKernelGGL((gn_stats_kernel<8>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((gn_stats_kernel<32>), grid, dim3(256), 0, s, a);
    }
    return hipGetLastError();
}

// ===========================================================================
// SABlock pre-norm: h[b,c,i] = LN_c(x[b,:,i]) * g[c] + b[c] + pe[i,c]
// one thread per token, channel loops are coalesced across the wave.
// ===========================================================================
__global__ __launch_bounds__(256) void ln_pe_kernel(LnPeArgs a) {
    // block = 64 tokens x 4 channel quarters: every load is a 256-byte run of tokens of one channel
    __shared__ float red[4][64];
    __shared__ float stat[2][64];
    const int lane = threadIdx.x & 63, qd = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + lane;
    const int b = blockIdx.y;
    const bool ok = i < a.n;
    const int cq = (a.C + 3) / 4, c_lo = qd * cq, c_hi = min(a.C, c_lo + cq);
    const float* xs = a.x + (long)b * a.x_bs + (ok ? i : 0);
    // C <= 128: the thread's quarter of the channel vector stays in registers -- ONE pass over x, all its loads (and those of
    // gamma / beta / the positional table) in flight together instead of three dependent sweeps (33 -> 9 us at 128 x 256)
    constexpr int CQ = 32;
    const bool in_regs = cq <= CQ;
    float xv[CQ];
    float s = 0.0f;
    if (in_regs) {
#pragma unroll
        for (int u = 0; u < CQ; ++u) xv[u] = c_lo + u < c_hi ? xs[(long)(c_lo + u) * a.n] : 0.0f;
#pragma unroll
        for (int u = 0; u < CQ; ++u) s += xv[u];            // (same order as the loop below)
    } else {
        for (int c = c_lo; c < c_hi; ++c) s += xs[(long)c * a.n];
    }
    red[qd][lane] = s;
    __syncthreads();
    if (qd == 0) stat[0][lane] = (red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane]) / (float)a.C;
    __syncthreads();
    const float mean = stat[0][lane];
    float q = 0.0f;
    if (in_regs) {
#pragma unroll
        for (int u = 0; u < CQ; ++u) {
            const float d = xv[u] - mean;
            q += c_lo + u < c_hi ? d * d : 0.0f;
        }
    } else {
        for (int c = c_lo; c < c_hi; ++c) {
            const float d = xs[(long)c * a.n] - mean;
            q += d * d;
        }
    }
    red[qd][lane] = q;
    __syncthreads();
    if (qd == 0)
        stat[1][lane] = 1.0f / sqrtf((red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane]) / (float)a.C + a.eps);
    __syncthreads();
    const float rstd = stat[1][lane];
    if (!ok) return;
    float* hs = a.h + (long)b * a.C * a.n + i;
    if (in_regs) {
        float ga[CQ], be[CQ], pe[CQ];
#pragma unroll
        for (int u = 0; u < CQ; ++u) {
            const int c = c_lo + u < c_hi ? c_lo + u : min(c_lo, a.C - 1);      // (a quarter past the last channel, C = 5: c_lo = 6)
            ga[u] = a.gamma[c]; be[u] = a.beta[c];
            pe[u] = a.pe_t ? a.pe_t[(long)c * a.pe_stride + i] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < CQ; ++u) {
            if (c_lo + u < c_hi) {
                float v = (xv[u] - mean) * rstd * ga[u] + be[u];
                if (a.pe_t) v += pe[u];
                hs[(long)(c_lo + u) * a.n] = v;
            }
        }
        return;
    }
    for (int c = c_lo; c < c_hi; ++c) {
        float v = (xs[(long)c * a.n] - mean) * rstd * a.gamma[c] + a.beta[c];
        if (a.pe_t) v += a.pe_t[(long)c * a.pe_stride + i];
        hs[(long)c * a.n] = v;
    }
}

hipError_t launch_ln_pe(const LnPeArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(ln_pe_kernel, dim3((a.n + 63) / 64, a.B), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ===========================================================================
// Softmax attention (SABlock core), flash-style online softmax on fp32 MFMA.
// Block = 4 waves = 128 queries of one (sample, head); K/V tiles of 32 keys go
// through LDS.  S^T = K^T Q puts the query on the lane, so the row softmax is
// lane-local (+ one cross-half shuffle) and the S^T accumulator is directly the
// B operand of O^T += V P^T (k-step r <-> accumulator register r; the A operand
// V is fetched in the matching permuted key order).
// ===========================================================================
template <int D>
__global__ __launch_bounds__(256) void attention_kernel(AttnArgs a) {
    __shared__ float Ks[D * 32];
    __shared__ float Vs[D * 33];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, kh = lane >> 5;
    const int h = blockIdx.y, b = blockIdx.z;
    const int n = a.n;
    const long inner = (long)a.heads * D;
    const float* qb = a.qkv + ((long)b * 3 * inner + (long)h * D) * n;
    const float* kb = qb + inner * n;
    const float* vb = kb + inner * n;
    const int query = (blockIdx.x * 4 + wave) * 32 + l31;
    const bool qvalid = query < n;

    float qreg[D / 2];
#pragma unroll
    for (int kk = 0; kk < D / 2; ++kk) qreg[kk] = qvalid ? qb[(long)(2 * kk + kh) * n + query] : 0.0f;

    float m = -INFINITY, l = 0.0f;
    f32x16 oacc[D / 32];
#pragma unroll
    for (int mt = 0; mt < D / 32; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[mt][r] = 0.0f;

    const int ntile = (n + 31) / 32;
    // K/V tile kt+1 is fetched into registers while tile kt is being used
    constexpr int NKV = D * 32 / 256;
    float kpre[NKV], vpre[NKV];
    auto fetch = [&](int kt) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < NKV; ++u) {
            const int i = tid + u * 256, d = i >> 5, key = kt * 32 + (i & 31);
            const bool kv = key < n;
            kpre[u] = kv ? kb[(long)d * n + key] : 0.0f;
            vpre[u] = kv ? vb[(long)d * n + key] : 0.0f;
        }
    };
    fetch(0);
    for (int kt = 0; kt < ntile; ++kt) {
        const int key0 = kt * 32;
        __syncthreads();
#pragma unroll
        for (int u = 0; u < NKV; ++u) {
            const int i = tid + u * 256, d = i >> 5, j = i & 31;
            Ks[d * 32 + j] = kpre[u];
            Vs[d * 33 + j] = vpre[u];
        }
        __syncthreads();
        if (kt + 1 < ntile) fetch(kt + 1);
        f32x16 sacc;
#pragma unroll
        for (int r = 0; r < 16; ++r) sacc[r] = 0.0f;
#pragma unroll
        for (int kk = 0; kk < D / 2; ++kk)
            sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(Ks[(2 * kk + kh) * 32 + l31], qreg[kk], sacc, 0, 0, 0);
        float tmax = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = key0 + drow(r, kh);
            float sv = sacc[r] * a.scale;
            if (key >= n) sv = -INFINITY;
            sacc[r] = sv;
            tmax = fmaxf(tmax, sv);
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
        const float mnew = fmaxf(m, tmax);
        const float alpha = __builtin_amdgcn_exp2f((m - mnew) * 1.44269504088896341f);   // v_exp_f32, not the library expf
        float lt = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float p = __builtin_amdgcn_exp2f((sacc[r] - mnew) * 1.44269504088896341f);
            sacc[r] = p;
            lt += p;
        }
        lt += __shfl_xor(lt, 32);
        l = l * alpha + lt;
        m = mnew;
#pragma unroll
        for (int mt = 0; mt < D / 32; ++mt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[mt][r] *= alpha;
#pragma unroll
            for (int r = 0; r < 16; ++r)
                oacc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(Vs[(mt * 32 + l31) * 33 + drow(r, kh)], sacc[r],
                                                                  oacc[mt], 0, 0, 0);
        }
    }
    if (qvalid) {
        const float inv = 1.0f / l;
        float* ob = a.o + ((long)b * inner + (long)h * D) * n + query;
#pragma unroll
        for (int mt = 0; mt < D / 32; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) ob[(long)(mt * 32 + drow(r, kh)) * n] = oacc[mt][r] * inv;
    }
}

// ---------------------------------------------------------------------------
// The same attention on the two-term fp16 split (f16x2): q, k, v multiplied by the power of two that puts the sample's
// max |qkv| (amax side channel of the qkv convolution) at [2^14, 2^15), the softmax weights (<= 1) by 2^14; three
// v_mfma_f32_32x32x16_f16 per product instead of eight v_mfma_f32_32x32x2_f32 (24 x 32 instead of 64 x 64 matrix
// cycles per 32-key tile and wave), one accumulator per tile.
//   S^T[key][query] = sum_d K[key][d] Q[d][query]: K tile in LDS as [key][d] (8 consecutive d per 16-byte unit), Q in
//        registers (lane = query, 8 consecutive d per k-step and lane half);
//   O^T[d][query] += sum_key V[d][key] P^T[key][query]: the S^T accumulator registers 8t'..8t'+7 of a lane half hold keys
//        16t' + 4kh + {0..3, 8..11}; V is stored with its keys permuted inside every 16-block so that these are 8
//        consecutive k positions of the A operand (the trick of the sandwich's second product), P is split in registers.
// ---------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256, 2) void attention_f_kernel(AttnArgs a) {
    constexpr int KW = D + 8, VW = 32 + 8;                  // row strides in fp16 elements (16-byte aligned rows)
    __shared__ __attribute__((aligned(16))) unsigned short Ks[2 * 32 * KW];     // [split][key][d]
    __shared__ __attribute__((aligned(16))) unsigned short Vs[2 * D * VW];      // [split][d][permuted key]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, kh = lane >> 5;
    const int h = blockIdx.y, b = blockIdx.z;
    const int n = a.n;
    const long inner = (long)a.heads * D;
    const float* qb = a.qkv + ((long)b * 3 * inner + (long)h * D) * n;
    const float* kb = qb + inner * n;
    const float* vb = kb + inner * n;
    const int query = (blockIdx.x * 4 + wave) * 32 + l31;
    const bool qvalid = query < n;
    float sinv;
    const float sc = f16x2_scale(amax_load(a.amax_in, b), sinv);       // one scale for q, k, v: max |qkv| of the sample
    constexpr float SP = 16384.0f, SPINV = 1.0f / 16384.0f;

    // Q: k-step t, lane half kh <-> d = 16t + 8kh + 0..7
    uint4 qh[D / 16], ql[D / 16];
    {
        float qv[D / 16][8];
#pragma unroll
        for (int t = 0; t < D / 16; ++t)
#pragma unroll
            for (int e = 0; e < 8; ++e) qv[t][e] = qvalid ? qb[(long)(16 * t + 8 * kh + e) * n + query] : 0.0f;
#pragma unroll
        for (int t = 0; t < D / 16; ++t) {
            unsigned hq[4], lq[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) split2_pair_f16(qv[t][2 * e] * sc, qv[t][2 * e + 1] * sc, hq[e], lq[e]);
            qh[t] = make_uint4(hq[0], hq[1], hq[2], hq[3]);
            ql[t] = make_uint4(lq[0], lq[1], lq[2], lq[3]);
        }
    }
    float m = -INFINITY, l = 0.0f;
    f32x16 oacc[D / 32];
#pragma unroll
    for (int mt = 0; mt < D / 32; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[mt][r] = 0.0f;

    const int ntile = (n + 31) / 32;
    // staging units: K -- (key = tid & 31, d octet = tid >> 5): 8 values strided by n; V -- (d = tid >> 2, key octet = tid & 3):
    // 8 consecutive keys.  D = 64: one unit of each per thread; D = 32: threads >= 128 idle.
    constexpr bool ALL = D == 64;
    const int kkey = tid & 31, koct = tid >> 5;
    const int vd = tid >> 2, voct = tid & 3;
    const bool kact = ALL || koct < D / 8, vact = ALL || vd < D;
    float kpre[8], vpre[8];
    auto fetch = [&](int kt) __attribute__((always_inline)) {
        const int key = kt * 32 + kkey;
#pragma unroll
        for (int e = 0; e < 8; ++e) kpre[e] = (kact && key < n) ? kb[(long)(8 * koct + e) * n + key] : 0.0f;
        const int k0 = kt * 32 + 8 * voct;
#pragma unroll
        for (int e = 0; e < 8; ++e) vpre[e] = (vact && k0 + e < n) ? vb[(long)vd * n + k0 + e] : 0.0f;
    };
    fetch(0);
    const char* ka = reinterpret_cast<const char*>(Ks) + (l31 * KW + 8 * kh) * 2;        // + s*32*KW*2 + t*32
    const char* va = reinterpret_cast<const char*>(Vs) + (l31 * VW + 8 * kh) * 2;        // + (s*D + mt*32)*VW*2 + t'*32
    for (int kt = 0; kt < ntile; ++kt) {
        const int key0 = kt * 32;
        __syncthreads();
        if (kact) {
            unsigned hq[4], lq[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) split2_pair_f16(kpre[2 * e] * sc, kpre[2 * e + 1] * sc, hq[e], lq[e]);
            *reinterpret_cast<uint4*>(Ks + (0 * 32 + kkey) * KW + 8 * koct) = make_uint4(hq[0], hq[1], hq[2], hq[3]);
            *reinterpret_cast<uint4*>(Ks + (1 * 32 + kkey) * KW + 8 * koct) = make_uint4(lq[0], lq[1], lq[2], lq[3]);
        }
        if (vact) {
            unsigned hq[4], lq[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) split2_pair_f16(vpre[2 * e] * sc, vpre[2 * e + 1] * sc, hq[e], lq[e]);
            // keys 8o..8o+3 and 8o+4..8o+7 of a 16-block go to positions (quad 0 -> 0, quad 1 -> 8, quad 2 -> 4, quad 3 -> 12)
            const int blk = (voct >> 1) * 16, p0 = blk + (voct & 1) * 4, p1 = p0 + 8;
            *reinterpret_cast<uint2*>(Vs + (0 * D + vd) * VW + p0) = make_uint2(hq[0], hq[1]);
            *reinterpret_cast<uint2*>(Vs + (0 * D + vd) * VW + p1) = make_uint2(hq[2], hq[3]);
            *reinterpret_cast<uint2*>(Vs + (1 * D + vd) * VW + p0) = make_uint2(lq[0], lq[1]);
            *reinterpret_cast<uint2*>(Vs + (1 * D + vd) * VW + p1) = make_uint2(lq[2], lq[3]);
        }
        __syncthreads();
        if (kt + 1 < ntile) fetch(kt + 1);
        f32x16 sacc;
#pragma unroll
        for (int r = 0; r < 16; ++r) sacc[r] = 0.0f;
#pragma unroll
        for (int t = 0; t < D / 16; ++t) {
            const f16x8 kh_ = *reinterpret_cast<const f16x8*>(ka + t * 32);
            const f16x8 kl_ = *reinterpret_cast<const f16x8*>(ka + 32 * KW * 2 + t * 32);
            sacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh_, __builtin_bit_cast(f16x8, qh[t]), sacc, 0, 0, 0);
            sacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh_, __builtin_bit_cast(f16x8, ql[t]), sacc, 0, 0, 0);
            sacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(kl_, __builtin_bit_cast(f16x8, qh[t]), sacc, 0, 0, 0);
        }
        const float sscale = (a.scale * sinv) * sinv;
        float tmax = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = key0 + drow(r, kh);
            float sv = sacc[r] * sscale;
            if (key >= n) sv = -INFINITY;
            sacc[r] = sv;
            tmax = fmaxf(tmax, sv);
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
        const float mnew = fmaxf(m, tmax);
        const float alpha = __builtin_amdgcn_exp2f((m - mnew) * 1.44269504088896341f);
        float lt = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float p = __builtin_amdgcn_exp2f((sacc[r] - mnew) * 1.44269504088896341f);
            sacc[r] = p;
            lt += p;
        }
        lt += __shfl_xor(lt, 32);
        l = l * alpha + lt;
        m = mnew;
        // P^T split in registers: k-step t' <-> accumulator registers 8t'..8t'+7
        uint4 ph[2], pl[2];
#pragma unroll
        for (int tp = 0; tp < 2; ++tp) {
            unsigned hq[4], lq[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) split2_pair_f16(sacc[8 * tp + 2 * e] * SP, sacc[8 * tp + 2 * e + 1] * SP, hq[e], lq[e]);
            ph[tp] = make_uint4(hq[0], hq[1], hq[2], hq[3]);
            pl[tp] = make_uint4(lq[0], lq[1], lq[2], lq[3]);
        }
        // the accumulator carries the factor sc * 2^14 of its operands; alpha rescales it like the plain one
#pragma unroll
        for (int mt = 0; mt < D / 32; ++mt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[mt][r] *= alpha;
#pragma unroll
            for (int tp = 0; tp < 2; ++tp) {
                const f16x8 vh_ = *reinterpret_cast<const f16x8*>(va + (0 * D + mt * 32) * (VW * 2) + tp * 32);
                const f16x8 vl_ = *reinterpret_cast<const f16x8*>(va + (1 * D + mt * 32) * (VW * 2) + tp * 32);
                oacc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh_, __builtin_bit_cast(f16x8, ph[tp]), oacc[mt], 0, 0, 0);
                oacc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh_, __builtin_bit_cast(f16x8, pl[tp]), oacc[mt], 0, 0, 0);
                oacc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vl_, __builtin_bit_cast(f16x8, ph[tp]), oacc[mt], 0, 0, 0);
            }
        }
    }
    if (qvalid) {
        const float inv = (SPINV * sinv) / l;
        float* ob = a.o + ((long)b * inner + (long)h * D) * n + query;
#pragma unroll
        for (int mt = 0; mt < D / 32; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) ob[(long)(mt * 32 + drow(r, kh)) * n] = oacc[mt][r] * inv;
    }
}

// f16x2 form where the producer recorded max |qkv| per sample (a per-layer condition); LNS_ATTN_FP32 keeps fp32 MFMA.
// Asked by launch_attention and by Planner::lower_sa (label, executed FLOP).
bool attn_is_f16(const AttnArgs& a) { return a.amax_in != nullptr && !knobs().attn_fp32; }

hipError_t launch_attention(const AttnArgs& a, hipStream_t s) {
    dim3 grid((a.n + 127) / 128, a.heads, a.B);
    if (attn_is_f16(a)) {
        if (a.D == 64) hipLaunchKernelGGL(attention_f_kernel<64>, grid, dim3(256), 0, s, a);
        else if (a.D == 32) hipLaunchKernelGGL(attention_f_kernel<32>, grid, dim3(256), 0, s, a);
        else return hipErrorInvalidValue;
        return hipGetLastError();
    }
    if (a.D == 64) hipLaunchKernelGGL(attention_kernel<64>, grid, dim3(256), 0, s, a);
    else if (a.D == 32) hipLaunchKernelGGL(attention_kernel<32>, grid, dim3(256), 0, s, a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

// ===========================================================================
// FABlock2D: axis pooling of the block's normalised input.  x [B,C,H,W] read through its per (sample, channel) GroupNorm
// (scale, shift) -> mx [B,H,C] = scale * mean over W + shift, my [B,W,C] = scale * mean over H + shift.  (to_in, a bias-free
// 1x1 conv, and the reducers' first Linear commute with the mean: they are applied to these rows as one matrix.)
// One block per (channel, sample); every row and every column is summed by one thread in ascending order, so the order
// is a function of (H, W) only.  (A form without the LDS copy -- a wave per row, butterfly row sums, per-wave column
// partials -- measured slower: 31.9 vs 19.2 us on the 64 x 64 block at B = 64)
// ===========================================================================
__global__ __launch_bounds__(256) void fa_pool_kernel(FaPoolArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* P = reinterpret_cast<float*>(smem);
    const int c = blockIdx.x, b = blockIdx.y;
    const int H = a.H, W = a.W, WP = W + 1;
    const float* vs = a.x + (long)b * a.x_bs + (long)c * H * W;
    float sc = 1.0f, sh = 0.0f;
    if (a.ss) { const float2 st = *reinterpret_cast<const float2*>(a.ss + ((long)b * a.C + c) * 2); sc = st.x; sh = st.y; }
    for (int i = threadIdx.x; i < H * W; i += 256) {
        const int y = i / W, x = i - y * W;
        P[y * WP + x] = vs[i];
    }
    __syncthreads();
    for (int y = threadIdx.x; y < H; y += 256) {
        float s = 0.0f;
        for (int x = 0; x < W; ++x) s += P[y * WP + x];
        a.mx[((long)b * H + y) * a.C + c] = fmaf(s / (float)W, sc, sh);
    }
    for (int x = threadIdx.x; x < W; x += 256) {
        float s = 0.0f;
        for (int y = 0; y < H; ++y) s += P[y * WP + x];
        a.my[((long)b * W + x) * a.C + c] = fmaf(s / (float)H, sc, sh);
    }
}

hipError_t launch_fa_pool(const FaPoolArgs& a, hipStream_t s) {
    const size_t lds = (size_t)a.H * (a.W + 1) * 4;
    hipLaunchKernelGGL(fa_pool_kernel, dim3(a.C, a.B), dim3(256), lds, s, a);
    return hipGetLastError();
}

// ===========================================================================
// FABlock2D PoolingReducer on pooled rows: to_in -> LayerNorm -> Linear ->
// GELU -> Linear(+bias).  8 rows per block so every weight is read once per 8
// rows; weights are stored in-major so lanes read consecutive outputs.
// ===========================================================================
#define FAR_ROWS 16
__global__ __launch_bounds__(256) void fa_reducer_kernel(FaReducerArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int C = a.C, Hid = a.Hid, Out = a.Out;
    float* w_in = reinterpret_cast<float*>(smem);     // [C][C]   in-major
    float* w1 = w_in + C * C;                         // [C][Hid]
    float* w2 = w1 + C * Hid;                         // [Hid][Out]
    float* vin = w2 + Hid * Out;                      // [R][C]
    float* t = vin + FAR_ROWS * C;                    // [R][C]
    float* hb = t + FAR_ROWS * C;                     // [R][Hid]
    const int tid = threadIdx.x;
    // all three weight matrices once per block, coalesced (they are re-used by 16 rows)
    for (int i = tid; i < C * C; i += 256) w_in[i] = a.win_t[i];
    for (int i = tid; i < C * Hid; i += 256) w1[i] = a.w1_t[i];
    for (int i = tid; i < Hid * Out; i += 256) w2[i] = a.w2_t[i];
    const long row0 = (long)blockIdx.x * FAR_ROWS;
    for (int i = tid; i < FAR_ROWS * C; i += 256) {
        const long row = row0 + i / C;
        vin[i] = row < a.rows ? a.m[row * C + (i % C)] : 0.0f;
    }
    __syncthreads();
    for (int idx = tid; idx < FAR_ROWS * C; idx += 256) {       // to_in
        const int r = idx / C, o = idx - r * C;
        float acc = 0.0f;
        for (int i = 0; i < C; ++i) acc += w_in[i * C + o] * vin[r * C + i];
        t[idx] = acc;
    }
    __syncthreads();
    if (tid < FAR_ROWS) {                                        // LayerNorm(C), eps 1e-5
        float s = 0.0f;
        for (int i = 0; i < C; ++i) s += t[tid * C + i];
        const float mean = s / (float)C;
        float q = 0.0f;
        for (int i = 0; i < C; ++i) { const float d = t[tid * C + i] - mean; q += d * d; }
        const float rstd = 1.0f / sqrtf(q / (float)C + 1e-5f);
        for (int i = 0; i < C; ++i) t[tid * C + i] = (t[tid * C + i] - mean) * rstd * a.ln_g[i] + a.ln_b[i];
    }
    __syncthreads();
    for (int idx = tid; idx < FAR_ROWS * Hid; idx += 256) {     // Linear(C, 2C) + GELU
        const int r = idx / Hid, j = idx - r * Hid;
        float acc = 0.0f;
        for (int i = 0; i < C; ++i) acc += w1[i * Hid + j] * t[r * C + i];
        hb[idx] = act_apply(acc, ACT_GELU);
    }
    __syncthreads();
    for (int idx = tid; idx < FAR_ROWS * Out; idx += 256) {     // Linear(2C, out) + bias
        const int r = idx / Out, o = idx - r * Out;
        float acc = a.b2[o];
        for (int j = 0; j < Hid; ++j) acc += w2[j * Out + o] * hb[r * Hid + j];
        const long row = row0 + r;
        if (row < a.rows) {
            const long bi = row / a.n, i = row - bi * a.n;
            a.u[(bi * Out + o) * a.n + i] = acc;
            if (a.amax_out) atomicMax(a.amax_out + bi * LNS_AMAX_SUB + (idx & (LNS_AMAX_SUB - 1)), abs_bits(acc));
        }
    }
}

// MFMA form (C and Hid multiples of 32): 32 pooled rows per block are the 32 "pixels" (MFMA columns) of three
// chained small GEMMs whose activations never leave LDS ([channel][row], so an accumulator tile is written
// back with one row per lane and read again as the next B operand); weights (in-major = [k][m]) are staged
// through one LDS region per GEMM, the last one in chunks of 128 outputs.
#define FARM_R 32
#define FARM_RP 33
static size_t fa_reducer_mfma_lds(int C, int Hid, int Out, bool fused_qk) {
    const size_t wt = std::max(std::max((size_t)C * Hid, (size_t)Hid * 128), (size_t)Out * 128);
    return (wt + ((size_t)2 * C + Hid + (fused_qk ? Out : 0)) * FARM_RP + 256) * 4;
}
static size_t fa_reducer_mfma_lds(const FaReducerArgs& a) { return fa_reducer_mfma_lds(a.C, a.Hid, a.Out, a.qk != nullptr); }
size_t fa_reducer_mfma_lds_bytes(int C, int Hid, int Out) { return fa_reducer_mfma_lds(C, Hid, Out, false); }
size_t fa_reducer_scalar_lds_bytes(int C, int Hid, int Out) {
    return ((size_t)C * C + (size_t)C * Hid + (size_t)Hid * Out + (size_t)FAR_ROWS * ((size_t)2 * C + Hid)) * 4;
}
static bool fa_reducer_mfma_shape(int C, int Hid, int Out) {
    return C % 32 == 0 && Hid % 32 == 0 && C <= 256 && fa_reducer_mfma_lds_bytes(C, Hid, Out) <= FA_AXIS_LDS_LIMIT;
}
bool fa_reducer_fits(int C, int Hid, int Out, bool merged) {
    if (C < 1 || Hid < 1 || Out < 1 || C > 65536 || Hid > 65536 || Out > 65536) return false;
    return fa_reducer_mfma_shape(C, Hid, Out) || (!merged && fa_reducer_scalar_lds_bytes(C, Hid, Out) <= FA_AXIS_LDS_LIMIT);
}

__device__ __forceinline__ void fa_reducer_mfma_body(const FaReducerArgs& a, int block, char* smem) {
    const int C = a.C, Hid = a.Hid, Out = a.Out;
    const int wt_floats = max(max(C * Hid, Hid * 128), Out * 128);
    float* Wt = reinterpret_cast<float*>(smem);           // current weight matrix / chunk, [k][m]
    float* X0 = Wt + wt_floats;                           // [C][RP]   pooled rows
    float* X1 = X0 + C * FARM_RP;                         // [C][RP]   to_in output / LayerNorm
    float* X2 = X1 + C * FARM_RP;                         // [Hid][RP] hidden
    float* red = X2 + Hid * FARM_RP;                      // [8][32] LayerNorm partials
    float* X3 = red + 256;                                // [Out][RP] reducer output (only with the fused to_qk)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, kh = lane >> 5;
    const long row0 = (long)block * FARM_R;

    // global -> LDS staging with 16 loads in flight per thread (a plain copy loop keeps one)
    auto stage = [&](float* dst, int n, auto src) __attribute__((always_inline)) {
        for (int base = 0; base < n; base += 256 * 16) {
            float v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) { const int i = base + tid + u * 256; v[u] = i < n ? src(i) : 0.0f; }
#pragma unroll
            for (int u = 0; u < 16; ++u) { const int i = base + tid + u * 256; if (i < n) dst[i] = v[u]; }
        }
    };
    stage(Wt, C * C, [&](int i) { return a.win_t[i]; });
    for (int base = 0; base < FARM_R * C; base += 256 * 8) {     // m[row][c] -> X0[c][r]
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = base + tid + u * 256, r = i / C, c = i - r * C;
            v[u] = (i < FARM_R * C && row0 + r < a.rows) ? a.m[(row0 + r) * C + c] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = base + tid + u * 256, r = i / C, c = i - r * C;
            if (i < FARM_R * C) X0[c * FARM_RP + r] = v[u];
        }
    }
    __syncthreads();
    // out[m][r] = sum_k W[k][m] * X[k][r] for the 32-row tile mt of W's columns
    auto gemm_tile = [&](const float* W, int ldw, int m0, const float* X, int K) __attribute__((always_inline)) -> f32x16 {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
        const float* wp = W + kh * ldw + m0 + l31;
        const float* xp = X + kh * FARM_RP + l31;
#pragma unroll 8
        for (int kk = 0; kk < K / 2; ++kk)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wp[2 * kk * ldw], xp[2 * kk * FARM_RP], acc, 0, 0, 0);
        return acc;
    };
    for (int mt = wave; mt < C / 32; mt += 4) {           // to_in
        const f32x16 acc = gemm_tile(Wt, C, mt * 32, X0, C);
#pragma unroll
        for (int r = 0; r < 16; ++r) X1[(mt * 32 + drow(r, kh)) * FARM_RP + l31] = acc[r];
    }
    __syncthreads();
    stage(Wt, C * Hid, [&](int i) { return a.w1_t[i]; });           // overlaps with the LayerNorm below
    {   // LayerNorm over channels, eps 1e-5 (two-pass): 8 partial sums per row
        const int r = tid & 31, part = tid >> 5, per = C / 8;
        float sacc = 0.0f;
        for (int i = part * per; i < (part + 1) * per; ++i) sacc += X1[i * FARM_RP + r];
        red[part * 32 + r] = sacc;
        __syncthreads();
        float mean = 0.0f;
#pragma unroll
        for (int p = 0; p < 8; ++p) mean += red[p * 32 + r];
        mean /= (float)C;
        __syncthreads();
        float q = 0.0f;
        for (int i = part * per; i < (part + 1) * per; ++i) { const float d = X1[i * FARM_RP + r] - mean; q += d * d; }
        red[part * 32 + r] = q;
        __syncthreads();
        float var = 0.0f;
#pragma unroll
        for (int p = 0; p < 8; ++p) var += red[p * 32 + r];
        const float rstd = 1.0f / sqrtf(var / (float)C + 1e-5f);
        for (int i = part * per; i < (part + 1) * per; ++i)
            X1[i * FARM_RP + r] = (X1[i * FARM_RP + r] - mean) * rstd * a.ln_g[i] + a.ln_b[i];
    }
    __syncthreads();
    for (int mt = wave; mt < Hid / 32; mt += 4) {         // Linear(C, Hid) + GELU
        const f32x16 acc = gemm_tile(Wt, Hid, mt * 32, X1, C);
#pragma unroll
        for (int r = 0; r < 16; ++r) X2[(mt * 32 + drow(r, kh)) * FARM_RP + l31] = act_apply(acc[r], ACT_GELU);
    }
    const long row = row0 + l31;
    const long bi = row / a.n, ii = row - bi * a.n;
    unsigned am_u = 0u;                                    // amax side channel: max |u| over this lane's row
    for (int o0 = 0; o0 < Out; o0 += 128) {                // Linear(Hid, Out) + bias, 128 outputs at a time
        __syncthreads();
        const int oc = min(128, Out - o0);
        stage(Wt, Hid * 128, [&](int i) {
            const int k = i >> 7, o = i & 127;
            return o < oc ? a.w2_t[(long)k * Out + o0 + o] : 0.0f;
        });
        __syncthreads();
        for (int mt = wave; mt * 32 < oc; mt += 4) {
            const f32x16 acc = gemm_tile(Wt, 128, mt * 32, X2, Hid);
            float b2v[16];                                 // bias loads batched ahead of the stores
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int o = o0 + mt * 32 + drow(r, kh);
                b2v[r] = a.b2[o < Out ? o : 0];
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int o = o0 + mt * 32 + drow(r, kh);
                if (o < Out) {
                    const float v = acc[r] + b2v[r];
                    if (a.u && row < a.rows) {
                        a.u[(bi * Out + o) * a.n + ii] = v;
                        am_u = max(am_u, abs_bits(v));
                    }
                    if (a.qk) X3[o * FARM_RP + l31] = v;
                }
            }
        }
    }
    if (a.amax_out) {
        // a block's 32 rows usually belong to one sample: one atomic per wave; otherwise one per lane
        const long bi0 = __builtin_amdgcn_readfirstlane((int)bi);
        const bool live = row < a.rows;
        const int sub = block & (LNS_AMAX_SUB - 1);
        if (__all((!live || bi == bi0) ? 1 : 0)) {
            const unsigned m = wave_umax(live ? am_u : 0u);
            if (lane == 0 && m) atomicMax(a.amax_out + bi0 * LNS_AMAX_SUB + sub, m);
        } else if (live) {
            atomicMax(a.amax_out + bi * LNS_AMAX_SUB + sub, am_u);
        }
    }
    if (a.qk) {                                            // fused to_qk: qk[m][r] = sum_o wqk[o][m] * X3[o][r] (+ bias)
        for (int m0 = 0; m0 < a.Mqk; m0 += 128) {
            __syncthreads();
            const int mc = min(128, a.Mqk - m0);
            stage(Wt, Out * 128, [&](int i) {
                const int k = i >> 7, o = i & 127;
                return o < mc ? a.wqk_t[(long)k * a.ldqk + m0 + o] : 0.0f;
            });
            __syncthreads();
            for (int mt = wave; mt * 32 < mc; mt += 4) {
                const f32x16 acc = gemm_tile(Wt, 128, mt * 32, X3, Out);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = m0 + mt * 32 + drow(r, kh);
                    if (m < a.Mqk && row < a.rows) a.qk[(bi * a.Mqk + m) * a.n + ii] = acc[r] + (a.bqk ? a.bqk[m] : 0.0f);
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void fa_reducer_mfma_kernel(FaReducerArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    fa_reducer_mfma_body(a, blockIdx.x, smem);
}

// both axes of a FABlock in one launch: the first nblk_x blocks run the x reducer, the rest the y reducer
__global__ __launch_bounds__(256) void fa_reducer2_mfma_kernel(FaReducerArgs ax, FaReducerArgs ay, int nblk_x) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if ((int)blockIdx.x < nblk_x) fa_reducer_mfma_body(ax, blockIdx.x, smem);
    else fa_reducer_mfma_body(ay, blockIdx.x - nblk_x, smem);
}

static bool fa_reducer_mfma_ok(const FaReducerArgs& a) {
    return fa_reducer_fits(a.C, a.Hid, a.Out, true) && (!a.qk || a.Out % 2 == 0) && fa_reducer_mfma_lds(a) <= FA_AXIS_LDS_LIMIT;
}

hipError_t launch_fa_reducer2(const FaReducerArgs& ax, const FaReducerArgs& ay, hipStream_t s) {
    if (!fa_reducer_mfma_ok(ax) || !fa_reducer_mfma_ok(ay)) return hipErrorInvalidValue;
    const size_t lds = std::max(fa_reducer_mfma_lds(ax), fa_reducer_mfma_lds(ay));
    const int nbx = (int)((ax.rows + FARM_R - 1) / FARM_R), nby = (int)((ay.rows + FARM_R - 1) / FARM_R);
    hipLaunchKernelGGL(fa_reducer2_mfma_kernel, dim3(nbx + nby), dim3(256), lds, s, ax, ay, nbx);
    return hipGetLastError();
}

hipError_t launch_fa_reducer(const FaReducerArgs& a, hipStream_t s) {
    const bool scalar_only = knobs().fa_reducer_scalar;   // A/B knob
    if (!fa_reducer_fits(a.C, a.Hid, a.Out, false)) return hipErrorInvalidValue;
    if (a.qk && !(fa_reducer_mfma_ok(a) && !scalar_only)) return hipErrorInvalidValue;   // the fused projection needs the MFMA form
    if (!scalar_only && fa_reducer_mfma_ok(a)) {
        const size_t lds = fa_reducer_mfma_lds(a);
        {
            const unsigned nb = (unsigned)((a.rows + FARM_R - 1) / FARM_R);
            hipLaunchKernelGGL(fa_reducer_mfma_kernel, dim3(nb), dim3(256), lds, s, a);
            return hipGetLastError();
        }
    }
    const size_t lds = fa_reducer_scalar_lds_bytes(a.C, a.Hid, a.Out);
    if (lds > FA_AXIS_LDS_LIMIT) return hipErrorInvalidValue;      // (reached with the A/B knob only: the predicate covers the rest)
    const unsigned nb = (unsigned)((a.rows + FAR_ROWS - 1) / FAR_ROWS);
    hipLaunchKernelGGL(fa_reducer_kernel, dim3(nb), dim3(256), lds, s, a);
    return hipGetLastError();
}

// ===========================================================================
// FABlock2D LowRankKernel: rotary embedding of q,k then K = q k^T per (b,head)
// (no softmax, no scaling).  q',k' staged in LDS as [d][n_pad]; MFMA tiles.
// ===========================================================================
__device__ __forceinline__ void fa_lrk_body(const FaLrkArgs& a, char* smem);

__global__ __launch_bounds__(256) void fa_lrk_kernel(FaLrkArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    fa_lrk_body(a, smem);
}

__global__ __launch_bounds__(256) void fa_lrk2_kernel(FaLrkArgs ax, FaLrkArgs ay) {   // blockIdx.z: axis
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (blockIdx.z == 0) fa_lrk_body(ax, smem);
    else fa_lrk_body(ay, smem);
}

__device__ __forceinline__ void fa_lrk_body(const FaLrkArgs& a, char* smem) {
    const int n = a.n, DK = a.DK, half = DK >> 1;
    const int nt = (n + 31) / 32, npad = nt * 32;
    float* qs = reinterpret_cast<float*>(smem);   // [DK][npad]
    float* ks = qs + (size_t)DK * npad;
    const int h = blockIdx.x, b = blockIdx.y;
    const float* qb = a.qk + ((long)b * 2 * a.heads * DK + (long)h * DK) * n;
    const float* kb = qb + (long)a.heads * DK * n;
    const int tid = threadIdx.x;
    // rotary embedding of q and k into LDS.  A thread takes the PAIR (d, d + half) of a position: both outputs need the
    // same two inputs and the same (cos, sin) entry, so every input is loaded once, every load is a run of consecutive
    // positions of one row (the table is frequency-major), and a thread's 40 loads are in flight together.
    for (int base = 0; base < half * npad; base += 256 * 8) {
        float c_[8], s_[8], q0[8], q1[8], k0[8], k1[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = base + tid + u * 256;
            const int d = i / npad, j = i - d * npad;
            const bool ok = i < half * npad && j < n;
            const int dd = ok ? d : 0, jj = ok ? j : 0;
            const float2 t = *reinterpret_cast<const float2*>(a.cs + ((long)dd * n + jj) * 2);
            c_[u] = t.x; s_[u] = t.y;
            q0[u] = qb[(long)dd * n + jj]; q1[u] = qb[(long)(dd + half) * n + jj];
            k0[u] = kb[(long)dd * n + jj]; k1[u] = kb[(long)(dd + half) * n + jj];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = base + tid + u * 256;
            const int d = i / npad, j = i - d * npad;
            if (i < half * npad) {
                const bool ok = j < n;
                qs[i] = ok ? q0[u] * c_[u] + -1.0f * q1[u] * s_[u] : 0.0f;                       // d < half
                ks[i] = ok ? k0[u] * c_[u] + -1.0f * k1[u] * s_[u] : 0.0f;
                qs[i + half * npad] = ok ? q1[u] * c_[u] + 1.0f * q0[u] * s_[u] : 0.0f;          // d + half
                ks[i + half * npad] = ok ? k1[u] * c_[u] + 1.0f * k0[u] * s_[u] : 0.0f;
            }
        }
    }
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6, l31 = lane & 31, kh = lane >> 5;
    float* ob = a.kmat + ((long)b * a.heads + h) * n * n;
    for (int tile = wave; tile < nt * nt; tile += 4) {
        const int it = tile / nt, jt = tile - it * nt;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
        const float* qp = qs + it * 32 + l31 + kh * npad;
        const float* kp = ks + jt * 32 + l31 + kh * npad;
#pragma unroll 8
        for (int kk = 0; kk < half; ++kk)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qp[2 * kk * npad], kp[2 * kk * npad], acc, 0, 0, 0);
        const int j = jt * 32 + l31;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = it * 32 + drow(r, kh);
            if (i < n && j < n) ob[(long)i * n + j] = acc[r];
        }
    }
}

size_t fa_lrk_lds_bytes(int DK, int n) { return (size_t)2 * DK * (((size_t)n + 31) / 32 * 32) * 4; }
bool fa_lrk_fits(int DK, int n) {
    return DK >= 2 && DK % 2 == 0 && DK <= 65536 && n >= 1 && n <= 65536 && fa_lrk_lds_bytes(DK, n) <= FA_AXIS_LDS_LIMIT;
}

hipError_t launch_fa_lrk2(const FaLrkArgs& ax, const FaLrkArgs& ay, hipStream_t s) {
    if (ax.heads != ay.heads || ax.B != ay.B || ax.DK != ay.DK) return hipErrorInvalidValue;
    if (!fa_lrk_fits(ax.DK, std::max(ax.n, ay.n))) return hipErrorInvalidValue;
    const size_t lds = fa_lrk_lds_bytes(ax.DK, std::max(ax.n, ay.n));
    hipLaunchKernelGGL(fa_lrk2_kernel, dim3(ax.heads, ax.B, 2), dim3(256), lds, s, ax, ay);
    return hipGetLastError();
}

hipError_t launch_fa_lrk(const FaLrkArgs& a, hipStream_t s) {
    if (!fa_lrk_fits(a.DK, a.n)) return hipErrorInvalidValue;
    const size_t lds = fa_lrk_lds_bytes(a.DK, a.n);
    hipLaunchKernelGGL(fa_lrk_kernel, dim3(a.heads, a.B), dim3(256), lds, s, a);
    return hipGetLastError();
}

// ===========================================================================
// FABlock2D core: every channel plane P (H x W) of head h becomes
//     Y = Kx[b,h] . (P . Ky[b,h]^T)          (then InstanceNorm over the plane)
// One wave per plane at a time.  U = P Ky^T keeps the plane row j in registers
// and the column l on lanes, i.e. exactly the B-operand layout of the second
// product Y = Kx U, so U never leaves registers; Y has columns on lanes ->
// 128-byte row-segment stores.  InstanceNorm (biased var) is computed from the
// accumulator registers (two-pass, exact) and applied before the store.
// ===========================================================================
template <int HT, int WT, bool VEC>
__global__ __launch_bounds__(256, (HT * WT >= 6 || (HT * WT >= 4 && !VEC) ? 1 : 2)) void fa_sandwich_kernel(FaSandwichArgs a, int planes_per_block) {   // (scalar-load form of the 64 x 64 planes: the whole register file instead of spills)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int HP = HT * 32 + 1, WP = WT * 32 + 1;
    // plane prefetch registers: one 64-lane wave moves a whole (padded) plane, 32 rows at a time
    constexpr int NPH = 32 * (WT * 32) / 64;               // floats per lane per 32-row band
    constexpr int NQH = VEC ? NPH / 4 : NPH;               // load instructions per lane per band
    float* Kxs = reinterpret_cast<float*>(smem);          // [HT*32][HP]
    float* Kys = Kxs + HT * 32 * HP;                      // [WT*32][WP]
    float* Pall = Kys + WT * 32 * WP;                     // 4 x [32][WP]  (one 32-row band per wave)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, kh = lane >> 5;
    const int H = a.H, W = a.W, C = a.C;
    const int h = blockIdx.y, b = blockIdx.z + a.b0;
    const float* kxg = a.kx + ((long)b * a.heads + h) * H * H;
    const float* kyg = a.ky + ((long)b * a.heads + h) * W * W;
    // staged with all loads of a thread in flight at once (a plain copy loop keeps one outstanding)
    {
        constexpr int NX = HT * 32 * (HT * 32) / 256, NY = WT * 32 * (WT * 32) / 256;
        float vx[NX], vy[NY];
#pragma unroll
        for (int u = 0; u < NX; ++u) {
            const int i = tid + u * 256, r = i / (HT * 32), c = i - r * (HT * 32);
            vx[u] = (r < H && c < H) ? kxg[(long)r * H + c] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < NY; ++u) {
            const int i = tid + u * 256, r = i / (WT * 32), c = i - r * (WT * 32);
            vy[u] = (r < W && c < W) ? kyg[(long)r * W + c] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < NX; ++u) {
            const int i = tid + u * 256, r = i / (HT * 32), c = i - r * (HT * 32);
            Kxs[r * HP + c] = vx[u];
        }
#pragma unroll
        for (int u = 0; u < NY; ++u) {
            const int i = tid + u * 256, r = i / (WT * 32), c = i - r * (WT * 32);
            Kys[r * WP + c] = vy[u];
        }
    }
    float* Ps = Pall + wave * (32 * WP);
    for (int i = lane; i < 32 * WP; i += 64) Ps[i] = 0.0f;   // column padding stays zero for every band
    __syncthreads();

    // per-lane offsets inside a 32-row band (the same for every band / plane)
    int soff[NQH], doff[NQH];
    {
        const int per_row = VEC ? W / 4 : W;
#pragma unroll
        for (int q = 0; q < NQH; ++q) {
            const int f = lane + 64 * q;
            const int r = f / per_row, c = (f - r * per_row) * (VEC ? 4 : 1);
            soff[q] = r < 32 ? r * W + c : -1;
            doff[q] = r * WP + c;
        }
    }
    // band-level pipeline: while the MFMAs of band jt run, the loads of the next band (same plane
    // or band 0 of this wave's next plane) are in flight in registers
    float pf[NPH];
    auto prefetch = [&](const float* pg, int jt) __attribute__((always_inline)) {
#pragma unroll
        for (int q = 0; q < NQH; ++q) {
            const bool ok = soff[q] >= 0 && (jt * 32 + soff[q] / W) < H;
            const int so = ok ? jt * 32 * W + soff[q] : 0;   // clamped: loads are unconditional
            if (VEC) {
                const float4 t = *reinterpret_cast<const float4*>(pg + so);
                pf[4 * q] = t.x; pf[4 * q + 1] = t.y; pf[4 * q + 2] = t.z; pf[4 * q + 3] = t.w;
            } else {
                pf[q] = pg[so];
            }
        }
    };

    const int c_begin = blockIdx.x * planes_per_block;
    const float inv_cnt = 1.0f / (float)(H * W);
    const long plane0 = ((long)b * a.heads + h) * C;
    int c = c_begin + wave;
    const int c_end = min(c_begin + planes_per_block, C);
    if (c < c_end) prefetch(a.u + (plane0 + c) * H * W, 0);
    const int kpairs = (W + 1) >> 1;
    for (; c < c_end; c += 4) {
        f32x16 Y[HT][WT];
#pragma unroll
        for (int i = 0; i < HT; ++i)
#pragma unroll
            for (int j = 0; j < WT; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) Y[i][j][r] = 0.0f;
#pragma unroll
        for (int jt = 0; jt < HT; ++jt) {
            // band jt of the plane: registers -> this wave's private LDS band (row-major, odd row
            // stride: the column reads below are bank-conflict free).  No block barrier: LDS
            // operations of one wave execute in order.
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int q = 0; q < NQH; ++q) {
                const bool ok = soff[q] >= 0 && (jt * 32 + soff[q] / W) < H;
                if (soff[q] >= 0) {          // slots past the 32-row band do not exist
                    if (VEC) {
                        Ps[doff[q]] = ok ? pf[4 * q] : 0.0f; Ps[doff[q] + 1] = ok ? pf[4 * q + 1] : 0.0f;
                        Ps[doff[q] + 2] = ok ? pf[4 * q + 2] : 0.0f; Ps[doff[q] + 3] = ok ? pf[4 * q + 3] : 0.0f;
                    } else {
                        Ps[doff[q]] = ok ? pf[q] : 0.0f;
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();
            if (jt + 1 < HT) prefetch(a.u + (plane0 + c) * H * W, jt + 1);
            else if (c + 4 < c_end) prefetch(a.u + (plane0 + c + 4) * H * W, 0);
#pragma unroll
            for (int lt = 0; lt < WT; ++lt) {
                f32x16 U;                                  // U[j][l] = sum_m P[j][m] Ky[l][m]
#pragma unroll
                for (int r = 0; r < 16; ++r) U[r] = 0.0f;
                const float* kyp = Kys + (lt * 32 + l31) * WP + kh;
                const float* pp = Ps + l31 * WP + kh;
#pragma unroll 8
                for (int kk = 0; kk < kpairs; ++kk)
                    U = __builtin_amdgcn_mfma_f32_32x32x2f32(pp[2 * kk], kyp[2 * kk], U, 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);   // bound the scheduler's LDS-read hoisting (registers)
                // Y[i][l] += sum_{j in band} Kx[i][j] U[j][l]: U's accumulator registers are the B operand
#pragma unroll
                for (int it = 0; it < HT; ++it) {
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        Y[it][lt] = __builtin_amdgcn_mfma_f32_32x32x2f32(
                            Kxs[(it * 32 + l31) * HP + jt * 32 + drow(r, kh)], U[r], Y[it][lt], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        float mean = 0.0f, rstd = 1.0f;
        if (a.instnorm) {
            float s = 0.0f;
#pragma unroll
            for (int it = 0; it < HT; ++it)
#pragma unroll
                for (int lt = 0; lt < WT; ++lt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const bool v = (it * 32 + drow(r, kh) < H) && (lt * 32 + l31 < W);
                        s += v ? Y[it][lt][r] : 0.0f;
                    }
            mean = wave_sum(s) * inv_cnt;
            float q = 0.0f;
#pragma unroll
            for (int it = 0; it < HT; ++it)
#pragma unroll
                for (int lt = 0; lt < WT; ++lt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const bool v = (it * 32 + drow(r, kh) < H) && (lt * 32 + l31 < W);
                        const float d = Y[it][lt][r] - mean;
                        q += v ? d * d : 0.0f;
                    }
            rstd = 1.0f / sqrtf(wave_sum(q) * inv_cnt + a.eps);
        }
        float* og = a.out + (plane0 + c) * H * W;
#pragma unroll
        for (int it = 0; it < HT; ++it)
#pragma unroll
            for (int lt = 0; lt < WT; ++lt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int i = it * 32 + drow(r, kh), l = lt * 32 + l31;
                    if (i < H && l < W) og[i * W + l] = (Y[it][lt][r] - mean) * rstd;
                }
    }
}

// ---------------------------------------------------------------------------
// The same sandwich on the bf16 matrix pipe (bf16x3 scheme of the convolution kernels): P, Ky, Kx and the
// intermediate U are split into three bf16 terms, six products per fp32 product, two accumulators.
//   LDS: Ky [split][l][m] and Kx [split][i][j'] as bf16 rows (+8 elements of row padding -> 16-byte aligned,
//        conflict-free b128 fragment reads), a private [split][32 rows][m] band of P per wave.
//   Kx is stored with its columns permuted inside every 16-block so that the 8 rows of U a lane half holds
//   in accumulator registers 8t'..8t'+7 (rows (e&3) + 8(e>>2) + 4kh + 16t') are 8 CONSECUTIVE k positions of
//   the A operand: U is split and packed in registers and is directly the B operand of Y += Kx U.
// ---------------------------------------------------------------------------
__device__ __forceinline__ unsigned short bf16_bits(float x) {
    return __builtin_bit_cast(unsigned short, (__bf16)x);
}
__device__ __forceinline__ void split3_scalar(float x, unsigned short& h, unsigned short& m, unsigned short& l) {
    h = bf16_bits(x);
    const float r1 = x - __uint_as_float((unsigned)h << 16);
    m = bf16_bits(r1);
    l = bf16_bits(r1 - __uint_as_float((unsigned)m << 16));
}

// FULL: H == 32 HT and W == 32 WT (the 32x32 and 64x64 planes of NS2d): the validity masks of the partial-tile form
// drop out at compile time (same additions in the same order: both forms agree bit for bit on such planes).
// NWV: waves per block (4; 3 where the LDS image of four private P bands does not fit: 48x96 planes).
// ULOOP: one column tile of U at a time (P fragments re-read per tile) instead of all WT at once -- the same
// additions in the same order, a third of the U / Ky-fragment registers: no spills on the 2x3-tile planes.
template <int HT, int WT, bool VEC, bool FULL = false, int NWV = 4, bool ULOOP = false>
__global__ __launch_bounds__(64 * NWV, 1) void fa_sandwich_b_kernel(FaSandwichArgs a, int planes_per_block) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int HB = HT * 32, WB = WT * 32, NTHR = 64 * NWV;
    constexpr int KXW = HB + 8, KYW = WB + 8;               // row strides in bf16 elements
    constexpr int NPH = 32 * WB / 64;                       // plane floats per lane per 32-row band
    constexpr int NQH = VEC ? NPH / 4 : NPH;
    unsigned short* Kxs = reinterpret_cast<unsigned short*>(smem);      // [3][HB][KXW]
    unsigned short* Kys = Kxs + 3 * HB * KXW;                           // [3][WB][KYW]
    unsigned short* Pall = Kys + 3 * WB * KYW;                          // NWV x [3][32][KYW]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, kh = lane >> 5;
    const int H = a.H, W = a.W, C = a.C;
    const int h = blockIdx.y, b = blockIdx.z + a.b0;
    const float* kxg = a.kx + ((long)b * a.heads + h) * H * H;
    const float* kyg = a.ky + ((long)b * a.heads + h) * W * W;
    {   // Kx (column-permuted) and Ky, split, all loads of a thread in flight at once
        constexpr int NX = (HB * HB + NTHR - 1) / NTHR, NY = (WB * WB + NTHR - 1) / NTHR;
        float vx[NX], vy[NY];
#pragma unroll
        for (int u = 0; u < NX; ++u) {
            const int i = tid + u * NTHR, r = i / HB, c = i - r * HB;
            vx[u] = (r < H && c < H) ? kxg[(long)r * H + c] : 0.0f;      // (r >= HB past the end of a ragged last slot: r >= H too)
        }
#pragma unroll
        for (int u = 0; u < NY; ++u) {
            const int i = tid + u * NTHR, r = i / WB, c = i - r * WB;
            vy[u] = (r < W && c < W) ? kyg[(long)r * W + c] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < NX; ++u) {
            const int i = tid + u * NTHR, r = i / HB, c = i - r * HB;
            if (i >= HB * HB) continue;
            const int w = c & 15;
            const int cp = (c & ~15) | (w & 3) | (((w >> 3) & 1) << 2) | (((w >> 2) & 1) << 3);
            unsigned short hh, mm, ll;
            split3_scalar(vx[u], hh, mm, ll);
            Kxs[(0 * HB + r) * KXW + cp] = hh; Kxs[(1 * HB + r) * KXW + cp] = mm; Kxs[(2 * HB + r) * KXW + cp] = ll;
        }
#pragma unroll
        for (int u = 0; u < NY; ++u) {
            const int i = tid + u * NTHR, r = i / WB, c = i - r * WB;
            if (i >= WB * WB) continue;
            unsigned short hh, mm, ll;
            split3_scalar(vy[u], hh, mm, ll);
            Kys[(0 * WB + r) * KYW + c] = hh; Kys[(1 * WB + r) * KYW + c] = mm; Kys[(2 * WB + r) * KYW + c] = ll;
        }
    }
    unsigned short* Ps = Pall + wave * (3 * 32 * KYW);
    for (int i = lane; i < 3 * 32 * KYW / 2; i += 64) reinterpret_cast<unsigned*>(Ps)[i] = 0u;   // K padding stays zero
    __syncthreads();

    int soff[NQH], doff[NQH];
    {
        const int per_row = VEC ? W / 4 : W;
#pragma unroll
        for (int q = 0; q < NQH; ++q) {
            const int f = lane + 64 * q;
            const int r = f / per_row, c = (f - r * per_row) * (VEC ? 4 : 1);
            soff[q] = r < 32 ? r * W + c : -1;
            doff[q] = r * KYW + c;
        }
    }
    float pf[NPH];
    auto prefetch = [&](const float* pg, int jt) __attribute__((always_inline)) {
#pragma unroll
        for (int q = 0; q < NQH; ++q) {
            const bool ok = FULL || (soff[q] >= 0 && (jt * 32 + soff[q] / W) < H);
            const int so = ok ? jt * 32 * W + soff[q] : 0;
            if (VEC) {
                const float4 t = *reinterpret_cast<const float4*>(pg + so);
                pf[4 * q] = t.x; pf[4 * q + 1] = t.y; pf[4 * q + 2] = t.z; pf[4 * q + 3] = t.w;
            } else {
                pf[q] = pg[so];
            }
        }
    };

    const int c_begin = blockIdx.x * planes_per_block;
    const float inv_cnt = 1.0f / (float)(H * W);
    const long plane0 = ((long)b * a.heads + h) * C;
    int c = c_begin + wave;
    const int c_end = min(c_begin + planes_per_block, C);
    if (c < c_end) prefetch(a.u + (plane0 + c) * H * W, 0);
    // fragment base addresses (bytes)
    const char* pa = reinterpret_cast<const char*>(Ps) + (l31 * KYW + 8 * kh) * 2;                  // + s*32*KYW*2 + t*32
    const char* kyb = reinterpret_cast<const char*>(Kys) + (l31 * KYW + 8 * kh) * 2;                // + (s*WB + lt*32)*KYW*2 + t*32
    const char* kxa = reinterpret_cast<const char*>(Kxs) + (l31 * KXW + 8 * kh) * 2;                // + (s*HB + it*32)*KXW*2 + (jt*32+16t')*2
    for (; c < c_end; c += NWV) {
        f32x16 Yh[HT][WT], Yl[HT][WT];
#pragma unroll
        for (int i = 0; i < HT; ++i)
#pragma unroll
            for (int j = 0; j < WT; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) { Yh[i][j][r] = 0.0f; Yl[i][j][r] = 0.0f; }
#pragma unroll
        for (int jt = 0; jt < HT; ++jt) {
            // band jt: registers -> split -> this wave's private LDS band.  LDS operations of one wave execute in order.
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int q = 0; q < NQH; ++q) {
                const bool ok = FULL || (soff[q] >= 0 && (jt * 32 + soff[q] / W) < H);
                if (FULL || soff[q] >= 0) {
                    if (VEC) {
                        unsigned h0, m0, l0, h1, m1, l1;
                        split3_pair(ok ? pf[4 * q] : 0.0f, ok ? pf[4 * q + 1] : 0.0f, h0, m0, l0);
                        split3_pair(ok ? pf[4 * q + 2] : 0.0f, ok ? pf[4 * q + 3] : 0.0f, h1, m1, l1);
                        *reinterpret_cast<uint2*>(Ps + 0 * 32 * KYW + doff[q]) = make_uint2(h0, h1);
                        *reinterpret_cast<uint2*>(Ps + 1 * 32 * KYW + doff[q]) = make_uint2(m0, m1);
                        *reinterpret_cast<uint2*>(Ps + 2 * 32 * KYW + doff[q]) = make_uint2(l0, l1);
                    } else {
                        unsigned short hh, mm, ll;
                        split3_scalar(ok ? pf[q] : 0.0f, hh, mm, ll);
                        Ps[0 * 32 * KYW + doff[q]] = hh; Ps[1 * 32 * KYW + doff[q]] = mm; Ps[2 * 32 * KYW + doff[q]] = ll;
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();
            if (jt + 1 < HT) prefetch(a.u + (plane0 + c) * H * W, jt + 1);
            else if (c + NWV < c_end) prefetch(a.u + (plane0 + c + NWV) * H * W, 0);
            // U[j][l] = sum_m P[j][m] Ky[l][m] for all WT column tiles at once: the P fragments are read once
            // per k-step and consecutive MFMAs go to different accumulators (no dependent back-to-back issue).
            // ULOOP: the same per column tile (UT = 1 tile in flight), see the template comment.
            constexpr int UT = ULOOP ? 1 : WT;
#pragma unroll
            for (int l0 = 0; l0 < WT; l0 += UT) {
            f32x16 Uh[UT], Ul[UT];
#pragma unroll
            for (int lt = 0; lt < UT; ++lt)
#pragma unroll
                for (int r = 0; r < 16; ++r) { Uh[lt][r] = 0.0f; Ul[lt][r] = 0.0f; }
#pragma unroll
            for (int t = 0; t < WB / 16; ++t) {
                bf16x8 A[3], Bq[UT][3];
#pragma unroll
                for (int s = 0; s < 3; ++s) {
                    A[s] = *reinterpret_cast<const bf16x8*>(pa + s * (32 * KYW * 2) + t * 32);
#pragma unroll
                    for (int lt = 0; lt < UT; ++lt)
                        Bq[lt][s] = *reinterpret_cast<const bf16x8*>(kyb + (s * WB + (l0 + lt) * 32) * (KYW * 2) + t * 32);
                }
#define LNS_SWU(ACC, SA, SB)                                                                          \
    _Pragma("unroll") for (int lt = 0; lt < UT; ++lt)                                                 \
        ACC[lt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[SA], Bq[lt][SB], ACC[lt], 0, 0, 0);
                LNS_SWU(Ul, 1, 1)
                LNS_SWU(Uh, 0, 0)
                LNS_SWU(Ul, 0, 2)
                LNS_SWU(Ul, 2, 0)
                LNS_SWU(Ul, 0, 1)
                LNS_SWU(Ul, 1, 0)
#undef LNS_SWU
            }
#pragma unroll
            for (int ul = 0; ul < UT; ++ul) {
                const int lt = l0 + ul;
                // split U in registers: k-step t' of the second product takes registers 8t'..8t'+7
                uint4 Bu[2][3];
#pragma unroll
                for (int tp = 0; tp < 2; ++tp) {
                    unsigned hq[4], mq[4], lq[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        split3_pair(Uh[ul][8 * tp + 2 * e] + Ul[ul][8 * tp + 2 * e],
                                    Uh[ul][8 * tp + 2 * e + 1] + Ul[ul][8 * tp + 2 * e + 1], hq[e], mq[e], lq[e]);
                    Bu[tp][0] = make_uint4(hq[0], hq[1], hq[2], hq[3]);
                    Bu[tp][1] = make_uint4(mq[0], mq[1], mq[2], mq[3]);
                    Bu[tp][2] = make_uint4(lq[0], lq[1], lq[2], lq[3]);
                }
                // Y[i][l] += sum_{j in band} Kx[i][j] U[j][l], all HT row tiles per k-step (independent accumulators)
#pragma unroll
                for (int tp = 0; tp < 2; ++tp) {
                    bf16x8 A[HT][3], Bq[3];
#pragma unroll
                    for (int s = 0; s < 3; ++s) {
#pragma unroll
                        for (int it = 0; it < HT; ++it)
                            A[it][s] = *reinterpret_cast<const bf16x8*>(kxa + (s * HB + it * 32) * (KXW * 2) + (jt * 32 + 16 * tp) * 2);
                        Bq[s] = __builtin_bit_cast(bf16x8, Bu[tp][s]);
                    }
#define LNS_SWY(ACC, SA, SB)                                                                          \
    _Pragma("unroll") for (int it = 0; it < HT; ++it)                                                 \
        ACC[it][lt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[it][SA], Bq[SB], ACC[it][lt], 0, 0, 0);
                    LNS_SWY(Yl, 1, 1)
                    LNS_SWY(Yh, 0, 0)
                    LNS_SWY(Yl, 0, 2)
                    LNS_SWY(Yl, 2, 0)
                    LNS_SWY(Yl, 0, 1)
                    LNS_SWY(Yl, 1, 0)
#undef LNS_SWY
                }
            }
            }   // l0
        }
#pragma unroll
        for (int it = 0; it < HT; ++it)
#pragma unroll
            for (int lt = 0; lt < WT; ++lt)
#pragma unroll
                for (int r = 0; r < 16; ++r) Yh[it][lt][r] += Yl[it][lt][r];
        float mean = 0.0f, rstd = 1.0f;
        if (a.instnorm) {
            float sacc = 0.0f;
#pragma unroll
            for (int it = 0; it < HT; ++it)
#pragma unroll
                for (int lt = 0; lt < WT; ++lt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const bool v = FULL || ((it * 32 + drow(r, kh) < H) && (lt * 32 + l31 < W));
                        sacc += v ? Yh[it][lt][r] : 0.0f;
                    }
            mean = wave_sum(sacc) * inv_cnt;
            float q = 0.0f;
#pragma unroll
            for (int it = 0; it < HT; ++it)
#pragma unroll
                for (int lt = 0; lt < WT; ++lt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const bool v = FULL || ((it * 32 + drow(r, kh) < H) && (lt * 32 + l31 < W));
                        const float d = Yh[it][lt][r] - mean;
                        q += v ? d * d : 0.0f;
                    }
            rstd = 1.0f / sqrtf(wave_sum(q) * inv_cnt + a.eps);
        }
        float* og = a.out + (plane0 + c) * H * W;
#pragma unroll
        for (int it = 0; it < HT; ++it)
#pragma unroll
            for (int lt = 0; lt < WT; ++lt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int i = it * 32 + drow(r, kh), l = lt * 32 + l31;
                    if (FULL || (i < H && l < W)) og[i * W + l] = (Yh[it][lt][r] - mean) * rstd;
                }
    }
}

// ---------------------------------------------------------------------------
// The sandwich on the two-term fp16 split (f16x2, the scheme of the convolution kernels): three products per fp32
// product instead of six, two split terms instead of three, 2/3 of the LDS image -- so TWO blocks fit a CU (74 KB at
// 64 x 64) where the bf16x3 form fits one.  Every operand is multiplied by a power of two that puts its bound at
// 2^14 <= . < 2^15 before the split:
//   P  : the sample's max |u| (amax side channel of the in_proj convolution, FaSandwichArgs::amax_u)
//   Kx, Ky : their own maxima over the (sample, head) matrix, reduced in the block prologue
//   U = P Ky^T : |U[j][l]| <= max|P| * max_l sum_m |Ky[l][m]| (largest absolute row sum of Ky, prologue as well) --
//        ONE scale for all bands of a plane, because the bands accumulate into the same Y accumulators
// All four are functions of the sample alone, never of the batch.  Two blocks per CU for W <= 64; the 48 x 96 planes of
// the SW decoder (WT = 3, 111 KB) run one block per CU with the whole register file.
// ---------------------------------------------------------------------------
template <int HT, int WT, bool VEC, bool FULL, bool ULOOP>
__global__ __launch_bounds__(256, (WT <= 2 && (VEC || HT * WT < 4) ? 2 : 1)) void fa_sandwich_f_kernel(FaSandwichArgs a, int planes_per_block) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int SPL = 2, NWV = 4;
    constexpr int HB = HT * 32, WB = WT * 32, NTHR = 64 * NWV;
    constexpr int KXW = HB + 8, KYW = WB + 8;               // row strides in fp16 elements
    constexpr int NPH = 32 * WB / 64;                       // plane floats per lane per 32-row band
    constexpr int NQH = VEC ? NPH / 4 : NPH;
    unsigned short* Kxs = reinterpret_cast<unsigned short*>(smem);      // [2][HB][KXW]
    unsigned short* Kys = Kxs + SPL * HB * KXW;                         // [2][WB][KYW]
    unsigned short* Pall = Kys + SPL * WB * KYW;                        // 4 x [2][32][KYW]
    unsigned* red = reinterpret_cast<unsigned*>(Pall + NWV * SPL * 32 * KYW);   // [4 waves][3]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, kh = lane >> 5;
    const int H = a.H, W = a.W, C = a.C;
    // samples in REVERSE launch order (a.b_rev): the producer (in_proj) wrote sample B-1 last and the consumer (to_out) reads
    // sample 0 first, so both hand-overs of the 537 MB tensor start on the end that is still in the Infinity Cache
    const int h = blockIdx.y, b = a.b0 + (a.b_rev ? a.B - 1 - (int)blockIdx.z : (int)blockIdx.z);
    const float* kxg = a.kx + ((long)b * a.heads + h) * H * H;
    const float* kyg = a.ky + ((long)b * a.heads + h) * W * W;
    float s_p, i_p, s_kx, i_kx, s_ky, i_ky, s_u, i_u;       // scales and their inverses (powers of two)
    {   // Kx (column-permuted) and Ky: all loads of a thread in flight at once, then the block-wide bounds, then the split
        constexpr int NX = (HB * HB + NTHR - 1) / NTHR, NY = (WB * WB + NTHR - 1) / NTHR;
        // threads per Ky row (a power of two, so that a row's threads are neighbouring lanes) and elements per thread
        constexpr int TPR = NTHR / WB >= 8 ? 8 : (NTHR / WB >= 4 ? 4 : 2), EPT = (WB + TPR - 1) / TPR;
        float vx[NX], vy[NY], rsv[EPT];
#pragma unroll
        for (int u = 0; u < NX; ++u) {
            const int i = tid + u * NTHR, r = i / HB, c = i - r * HB;
            vx[u] = (r < H && c < H) ? kxg[(long)r * H + c] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < NY; ++u) {
            const int i = tid + u * NTHR, r = i / WB, c = i - r * WB;
            vy[u] = (r < W && c < W) ? kyg[(long)r * W + c] : 0.0f;
        }
        {
            const int r = tid / TPR, q = tid - r * TPR;
#pragma unroll
            for (int e = 0; e < EPT; ++e) {
                const int c = q * EPT + e;
                rsv[e] = (r < W && c < W) ? kyg[(long)r * W + c] : 0.0f;
            }
        }
        unsigned mx = 0u, my = 0u;
#pragma unroll
        for (int u = 0; u < NX; ++u) mx = max(mx, abs_bits(vx[u]));
#pragma unroll
        for (int u = 0; u < NY; ++u) my = max(my, abs_bits(vy[u]));
        float rs = 0.0f;
#pragma unroll
        for (int e = 0; e < EPT; ++e) rs += fabsf(rsv[e]);
#pragma unroll
        for (int d = 1; d < TPR; d <<= 1) rs += __shfl_xor(rs, d);        // fixed order: the same sum on every lane of the row
        mx = wave_umax(mx); my = wave_umax(my);
        const unsigned mr = wave_umax(__float_as_uint(rs));
        if (lane == 0) { red[wave * 3] = mx; red[wave * 3 + 1] = my; red[wave * 3 + 2] = mr; }
        __syncthreads();
        const unsigned bx = max(max(red[0], red[3]), max(red[6], red[9]));
        const unsigned by = max(max(red[1], red[4]), max(red[7], red[10]));
        const unsigned br = max(max(red[2], red[5]), max(red[8], red[11]));
        const unsigned bp = amax_load(a.amax_u, b);
        s_kx = f16x2_scale(bx, i_kx);
        s_ky = f16x2_scale(by, i_ky);
        s_p = f16x2_scale(bp, i_p);
        s_u = f16x2_scale(__float_as_uint(__uint_as_float(bp) * __uint_as_float(br)), i_u);
#pragma unroll
        for (int u = 0; u < NX; ++u) {
            const int i = tid + u * NTHR, r = i / HB, c = i - r * HB;
            if (i >= HB * HB) continue;
            const int w = c & 15;
            const int cp = (c & ~15) | (w & 3) | (((w >> 3) & 1) << 2) | (((w >> 2) & 1) << 3);
            const float v = vx[u] * s_kx;
            const _Float16 hh = (_Float16)v, ll = (_Float16)(v - (float)hh);
            Kxs[(0 * HB + r) * KXW + cp] = __builtin_bit_cast(unsigned short, hh);
            Kxs[(1 * HB + r) * KXW + cp] = __builtin_bit_cast(unsigned short, ll);
        }
#pragma unroll
        for (int u = 0; u < NY; ++u) {
            const int i = tid + u * NTHR, r = i / WB, c = i - r * WB;
            if (i >= WB * WB) continue;
            const float v = vy[u] * s_ky;
            const _Float16 hh = (_Float16)v, ll = (_Float16)(v - (float)hh);
            Kys[(0 * WB + r) * KYW + c] = __builtin_bit_cast(unsigned short, hh);
            Kys[(1 * WB + r) * KYW + c] = __builtin_bit_cast(unsigned short, ll);
        }
    }
    unsigned short* Ps = Pall + wave * (SPL * 32 * KYW);
    for (int i = lane; i < SPL * 32 * KYW / 2; i += 64) reinterpret_cast<unsigned*>(Ps)[i] = 0u;   // K padding stays zero
    __syncthreads();

    int soff[NQH], doff[NQH];
    {
        const int per_row = VEC ? W / 4 : W;
#pragma unroll
        for (int q = 0; q < NQH; ++q) {
            const int f = lane + 64 * q;
            const int r = f / per_row, c = (f - r * per_row) * (VEC ? 4 : 1);
            soff[q] = r < 32 ? r * W + c : -1;
            doff[q] = r * KYW + c;
        }
    }
    float pf[NPH];
    auto prefetch = [&](const float* pg, int jt) __attribute__((always_inline)) {
#pragma unroll
        for (int q = 0; q < NQH; ++q) {
            const bool ok = FULL || (soff[q] >= 0 && (jt * 32 + soff[q] / W) < H);
            const int so = ok ? jt * 32 * W + soff[q] : 0;
            if (VEC) {
                const float4 t = *reinterpret_cast<const float4*>(pg + so);
                pf[4 * q] = t.x; pf[4 * q + 1] = t.y; pf[4 * q + 2] = t.z; pf[4 * q + 3] = t.w;
            } else {
                pf[q] = pg[so];
            }
        }
    };

    const int c_begin = blockIdx.x * planes_per_block;
    const float inv_cnt = 1.0f / (float)(H * W);
    const long plane0 = ((long)b * a.heads + h) * C;
    int c = c_begin + wave;
    const int c_end = min(c_begin + planes_per_block, C);
    if (c < c_end) prefetch(a.u + (plane0 + c) * H * W, 0);
    const char* pa = reinterpret_cast<const char*>(Ps) + (l31 * KYW + 8 * kh) * 2;                  // + s*32*KYW*2 + t*32
    const char* kyb = reinterpret_cast<const char*>(Kys) + (l31 * KYW + 8 * kh) * 2;                // + (s*WB + lt*32)*KYW*2 + t*32
    const char* kxa = reinterpret_cast<const char*>(Kxs) + (l31 * KXW + 8 * kh) * 2;                // + (s*HB + it*32)*KXW*2 + (jt*32+16t')*2
    for (; c < c_end; c += NWV) {
        // one accumulator per tile for all three products (hh' + hl' + lh'): the cross terms are 2^-11 of the main one,
        // adding them into the same fp32 accumulator costs what any fp32 chain costs -- and halves the registers, which
        // is what lets two waves share a SIMD
        f32x16 Yh[HT][WT];
#pragma unroll
        for (int i = 0; i < HT; ++i)
#pragma unroll
            for (int j = 0; j < WT; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) Yh[i][j][r] = 0.0f;
#pragma unroll
        for (int jt = 0; jt < HT; ++jt) {
            // band jt: registers -> scale, split -> this wave's private LDS band.  LDS operations of one wave execute in order.
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int q = 0; q < NQH; ++q) {
                const bool ok = FULL || (soff[q] >= 0 && (jt * 32 + soff[q] / W) < H);
                if (FULL || soff[q] >= 0) {
                    if (VEC) {
                        unsigned h0, l0, h1, l1;
                        split2_pair_f16(ok ? pf[4 * q] * s_p : 0.0f, ok ? pf[4 * q + 1] * s_p : 0.0f, h0, l0);
                        split2_pair_f16(ok ? pf[4 * q + 2] * s_p : 0.0f, ok ? pf[4 * q + 3] * s_p : 0.0f, h1, l1);
                        *reinterpret_cast<uint2*>(Ps + 0 * 32 * KYW + doff[q]) = make_uint2(h0, h1);
                        *reinterpret_cast<uint2*>(Ps + 1 * 32 * KYW + doff[q]) = make_uint2(l0, l1);
                    } else {
                        const float v = ok ? pf[q] * s_p : 0.0f;
                        const _Float16 hh = (_Float16)v, ll = (_Float16)(v - (float)hh);
                        Ps[0 * 32 * KYW + doff[q]] = __builtin_bit_cast(unsigned short, hh);
                        Ps[1 * 32 * KYW + doff[q]] = __builtin_bit_cast(unsigned short, ll);
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();
            if (jt + 1 < HT) prefetch(a.u + (plane0 + c) * H * W, jt + 1);
            else if (c + NWV < c_end) prefetch(a.u + (plane0 + c + NWV) * H * W, 0);
            constexpr int UT = ULOOP ? 1 : WT;
#pragma unroll
            for (int l0 = 0; l0 < WT; l0 += UT) {
                // U[j][l] = sum_m P[j][m] Ky[l][m]
                f32x16 Uh[UT];
#pragma unroll
                for (int lt = 0; lt < UT; ++lt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) Uh[lt][r] = 0.0f;
#pragma unroll
                for (int t = 0; t < WB / 16; ++t) {
                    f16x8 A[SPL], Bq[UT][SPL];
#pragma unroll
                    for (int s = 0; s < SPL; ++s) {
                        A[s] = *reinterpret_cast<const f16x8*>(pa + s * (32 * KYW * 2) + t * 32);
#pragma unroll
                        for (int lt = 0; lt < UT; ++lt)
                            Bq[lt][s] = *reinterpret_cast<const f16x8*>(kyb + (s * WB + (l0 + lt) * 32) * (KYW * 2) + t * 32);
                    }
#pragma unroll
                    for (int lt = 0; lt < UT; ++lt) Uh[lt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[0], Bq[lt][0], Uh[lt], 0, 0, 0);
#pragma unroll
                    for (int lt = 0; lt < UT; ++lt) Uh[lt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[0], Bq[lt][1], Uh[lt], 0, 0, 0);
#pragma unroll
                    for (int lt = 0; lt < UT; ++lt) Uh[lt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[1], Bq[lt][0], Uh[lt], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);       // one k-step of fragments in registers at a time (register budget of two waves per SIMD)
                }
#pragma unroll
                for (int ul = 0; ul < UT; ++ul) {
                    const int lt = l0 + ul;
                    // U back to its true scale, then to the scale of its bound; split in registers: k-step t' of the
                    // second product takes registers 8t'..8t'+7
                    uint4 Bu[2][SPL];
#pragma unroll
                    for (int tp = 0; tp < 2; ++tp) {
                        unsigned hq[4], lq[4];
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const float u0 = ((Uh[ul][8 * tp + 2 * e] * i_p) * i_ky) * s_u;
                            const float u1 = ((Uh[ul][8 * tp + 2 * e + 1] * i_p) * i_ky) * s_u;
                            split2_pair_f16(u0, u1, hq[e], lq[e]);
                        }
                        Bu[tp][0] = make_uint4(hq[0], hq[1], hq[2], hq[3]);
                        Bu[tp][1] = make_uint4(lq[0], lq[1], lq[2], lq[3]);
                    }
                    // Y[i][l] += sum_{j in band} Kx[i][j] U[j][l]
#pragma unroll
                    for (int tp = 0; tp < 2; ++tp) {
                        f16x8 A[HT][SPL], Bq[SPL];
#pragma unroll
                        for (int s = 0; s < SPL; ++s) {
#pragma unroll
                            for (int it = 0; it < HT; ++it)
                                A[it][s] = *reinterpret_cast<const f16x8*>(kxa + (s * HB + it * 32) * (KXW * 2) + (jt * 32 + 16 * tp) * 2);
                            Bq[s] = __builtin_bit_cast(f16x8, Bu[tp][s]);
                        }
#pragma unroll
                        for (int it = 0; it < HT; ++it) Yh[it][lt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[it][0], Bq[0], Yh[it][lt], 0, 0, 0);
#pragma unroll
                        for (int it = 0; it < HT; ++it) Yh[it][lt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[it][0], Bq[1], Yh[it][lt], 0, 0, 0);
#pragma unroll
                        for (int it = 0; it < HT; ++it) Yh[it][lt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[it][1], Bq[0], Yh[it][lt], 0, 0, 0);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            }   // l0
        }
#pragma unroll
        for (int it = 0; it < HT; ++it)
#pragma unroll
            for (int lt = 0; lt < WT; ++lt)
#pragma unroll
                for (int r = 0; r < 16; ++r) Yh[it][lt][r] = (Yh[it][lt][r] * i_kx) * i_u;
        float mean = 0.0f, rstd = 1.0f;
        if (a.instnorm) {
            float sacc = 0.0f;
#pragma unroll
            for (int it = 0; it < HT; ++it)
#pragma unroll
                for (int lt = 0; lt < WT; ++lt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const bool v = FULL || ((it * 32 + drow(r, kh) < H) && (lt * 32 + l31 < W));
                        sacc += v ? Yh[it][lt][r] : 0.0f;
                    }
            mean = wave_sum(sacc) * inv_cnt;
            float q = 0.0f;
#pragma unroll
            for (int it = 0; it < HT; ++it)
#pragma unroll
                for (int lt = 0; lt < WT; ++lt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const bool v = FULL || ((it * 32 + drow(r, kh) < H) && (lt * 32 + l31 < W));
                        const float d = Yh[it][lt][r] - mean;
                        q += v ? d * d : 0.0f;
                    }
            rstd = 1.0f / sqrtf(wave_sum(q) * inv_cnt + a.eps);
        }
        // stores through a buffer descriptor of the plane (its base made provably wave-uniform): the lane's offset in one
        // VGPR, the row offset in an SGPR -- per-element 64-bit addresses would cost 128 registers here
        float* og = a.out + (plane0 + c) * H * W;
        const unsigned long long ogp = reinterpret_cast<unsigned long long>(og);
        const unsigned og_lo = __builtin_amdgcn_readfirstlane((unsigned)ogp), og_hi = __builtin_amdgcn_readfirstlane((unsigned)(ogp >> 32));
        const __amdgpu_buffer_rsrc_t orr = __builtin_amdgcn_make_buffer_rsrc(
            reinterpret_cast<void*>(((unsigned long long)og_hi << 32) | og_lo), 0, H * W * 4, 0x00020000);
        const int vo = (4 * kh * W + l31) * 4;
#pragma unroll
        for (int it = 0; it < HT; ++it)
#pragma unroll
            for (int lt = 0; lt < WT; ++lt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int so = ((it * 32 + (r & 3) + 8 * (r >> 2)) * W + lt * 32) * 4;      // uniform
                    const float v = (Yh[it][lt][r] - mean) * rstd;
                    if (FULL) {
                        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), orr, vo, so, LNS_SAND_STORE_AUX);
                    } else {        // ragged plane: the range check masks (the row offset in the VGPR, invalid lanes at 2^31)
                        const int i = it * 32 + drow(r, kh), l = lt * 32 + l31;
                        const unsigned vr = (i < H && l < W) ? (unsigned)(vo + so) : 0x80000000u;
                        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), orr, (int)vr, 0, LNS_SAND_STORE_AUX);
                    }
                }
    }
}
static size_t fa_sandwich_f_lds_bytes(int HT, int WT) {
    const size_t HB = HT * 32, WB = WT * 32;
    return (2 * HB * (HB + 8) + 2 * WB * (WB + 8) + (size_t)4 * 2 * 32 * (WB + 8)) * 2 + 64;
}

#include "fa_fused.inc"

constexpr size_t fa_sandwich_b_lds_const(int HT, int WT, int nwv) {
    return ((size_t)3 * HT * 32 * (HT * 32 + 8) + (size_t)3 * WT * 32 * (WT * 32 + 8) + (size_t)nwv * 3 * 32 * (WT * 32 + 8)) * 2;
}
size_t fa_sandwich_lds_bytes(int H, int W) {
    const int HT = (H + 31) / 32, WT = (W + 31) / 32;
    const size_t HP = HT * 32 + 1, WP = WT * 32 + 1;
    return (HT * 32 * HP + WT * 32 * WP + 4 * 32 * WP) * 4;
}

// Which kernel a plain sandwich launch runs: a function of the plane (H, W), of whether the producer recorded max |u| and of the
// process switches -- never of the batch.  Asked by launch_fa_sandwich and by Planner::lower_fa (label, executed FLOP, refusal).
FaSandwichForm fa_sandwich_form(const FaSandwichArgs& a) {
    const Knobs& k = knobs();
    const int HT = (a.H + 31) / 32, WT = (a.W + 31) / 32;
    // the plane tilings the kernels are instantiated for: 32x32, 32x64, 64x64, 64x96, 64x32
    if (!((HT == 1 && (WT == 1 || WT == 2)) || (HT == 2 && WT >= 1 && WT <= 3))) return FA_SAND_NONE;
    if (!k.fa_sandwich_fp32) {
        // f16x2 form: planes of <= 96 columns whose producer recorded max |u| per sample (a per-layer condition)
        if (WT <= 3 && !k.fa_sandwich_bf16x3 && a.amax_u != nullptr && fa_sandwich_f_lds_bytes(HT, WT) <= 160 * 1024) return FA_SAND_F16X2;
        // bf16x3 form whenever its LDS image fits, four waves per block.  Where four private P bands do not fit the LDS (48x96
        // planes of the SW decoder: 167 KB) the three-wave form exists (NWV = 3, per-tile U) but measured SLOWER than the
        // fp32-MFMA kernel (SW 96x192x5, B=64: sandwich class 82.0 vs 69.8 ms per rollout -- 46 spilled registers, three waves
        // per CU), so LNS_FA_SANDWICH_3WAVE opts in and the default for those planes stays fp32 MFMA.
        const int nwv = fa_sandwich_b_lds_const(HT, WT, 4) <= 160 * 1024 ? 4 : 3;
        if ((nwv == 4 || k.fa_sandwich_3wave) && fa_sandwich_b_lds_const(HT, WT, nwv) <= 160 * 1024)
            return nwv == 4 ? FA_SAND_BF16X3 : FA_SAND_BF16X3_3WAVE;
    }
    return fa_sandwich_lds_bytes(a.H, a.W) <= 160 * 1024 ? FA_SAND_FP32 : FA_SAND_NONE;
}

template <int HT, int WT>
static hipError_t launch_fa_sandwich_t(const FaSandwichArgs& a, FaSandwichForm form, hipStream_t s) {
    constexpr int NWV = fa_sandwich_b_lds_const(HT, WT, 4) <= 160 * 1024 ? 4 : 3;      // (fa_sandwich_form's nwv)
    constexpr bool UL = HT * WT >= 6;
    const bool vec = (a.W % 4 == 0) && ((reinterpret_cast<uintptr_t>(a.u) & 15) == 0);
    // planes per block: the Kx/Ky staging (load + split) is paid once per block, so as many planes as still leave `want` blocks
    // (>= 2 per CU; fp32: enough blocks to fill the chip, few enough to amortise the staging)
    auto planes_per_block = [&](int ppb, long want) {
        while (ppb > 4 && (long)a.B * a.heads * ((a.C + ppb - 1) / ppb) < want) ppb >>= 1;
        return ppb;
    };
    const int ppb = form == FA_SAND_FP32 ? planes_per_block(16, 512) : planes_per_block((int)knobs().fa_ppb, form == FA_SAND_F16X2 ? 1024 : 512);
    const dim3 grid((a.C + ppb - 1) / ppb, a.heads, a.B);
    const bool full = vec && HT == WT && a.H == HT * 32 && a.W == WT * 32;       // layer-static: the shape decides, never the batch
    switch (form) {
        case FA_SAND_F16X2: {
            const size_t ldsf = fa_sandwich_f_lds_bytes(HT, WT);
            constexpr bool ULF = false;
            if (full) hipLaunchKernelGGL((fa_sandwich_f_kernel<HT, WT, true, (HT == WT), ULF>), grid, dim3(256), ldsf, s, a, ppb);
            else if (vec) hipLaunchKernelGGL((fa_sandwich_f_kernel<HT, WT, true, false, ULF>), grid, dim3(256), ldsf, s, a, ppb);
            else hipLaunchKernelGGL((fa_sandwich_f_kernel<HT, WT, false, false, ULF>), grid, dim3(256), ldsf, s, a, ppb);
            return hipGetLastError();
        }
        case FA_SAND_BF16X3:
        case FA_SAND_BF16X3_3WAVE: {
            const size_t ldsb = fa_sandwich_b_lds_const(HT, WT, NWV);
            if (full) hipLaunchKernelGGL((fa_sandwich_b_kernel<HT, WT, true, (HT == WT), NWV, UL>), grid, dim3(64 * NWV), ldsb, s, a, ppb);
            else if (vec) hipLaunchKernelGGL((fa_sandwich_b_kernel<HT, WT, true, false, NWV, UL>), grid, dim3(64 * NWV), ldsb, s, a, ppb);
            else hipLaunchKernelGGL((fa_sandwich_b_kernel<HT, WT, false, false, NWV, UL>), grid, dim3(64 * NWV), ldsb, s, a, ppb);
            return hipGetLastError();
        }
        case FA_SAND_FP32: {
            const size_t lds = fa_sandwich_lds_bytes(a.H, a.W);
            if (vec) hipLaunchKernelGGL((fa_sandwich_kernel<HT, WT, true>), grid, dim3(256), lds, s, a, ppb);
            else hipLaunchKernelGGL((fa_sandwich_kernel<HT, WT, false>), grid, dim3(256), lds, s, a, ppb);
            return hipGetLastError();
        }
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_fa_sandwich(const FaSandwichArgs& a, hipStream_t s) {
    const FaSandwichForm form = fa_sandwich_form(a);
    const int HT = (a.H + 31) / 32, WT = (a.W + 31) / 32;
    if (form == FA_SAND_NONE) return hipErrorInvalidValue;
    if (HT == 1 && WT == 1) return launch_fa_sandwich_t<1, 1>(a, form, s);
    if (HT == 1 && WT == 2) return launch_fa_sandwich_t<1, 2>(a, form, s);
    if (HT == 2 && WT == 2) return launch_fa_sandwich_t<2, 2>(a, form, s);
    if (HT == 2 && WT == 3) return launch_fa_sandwich_t<2, 3>(a, form, s);
    return launch_fa_sandwich_t<2, 1>(a, form, s);
}

// ===========================================================================
// Conditional propagator: per-sample embedding MLPs.  One block per sample; the
// vectors are <= 128 long, the matrices are stored in-major so lanes read
// consecutive outputs.  train_stage2_twophase_conditional.py:66-75,114-116,
// modules/cond_utils.py:19-38.
// ===========================================================================
__global__ __launch_bounds__(128) void cond_base_kernel(CondBaseArgs a) {
    __shared__ float v0[256], v1[256];
    const int b = blockIdx.x, tid = threadIdx.x, E = a.E, half = E / 2;
    const float t = a.param[b];
    for (int i = tid; i < E; i += 128) {
        float val = 0.0f;
        if (i < half) val = cosf(t * a.freqs[i]);
        else if (i < 2 * half) val = sinf(t * a.freqs[i - half]);
        v0[i] = val;
    }
    __syncthreads();
    const int Hd = a.Hd > 0 ? a.Hd : E;
    for (int o = tid; o < Hd; o += 128) {
        float acc = a.b0[o];
        for (int i = 0; i < E; ++i) acc += a.w0_t[i * Hd + o] * v0[i];
        v1[o] = act_apply(acc, a.act ? a.act : ACT_GELU);
    }
    __syncthreads();
    for (int o = tid; o < E; o += 128) {
        float acc = a.b2[o];
        for (int i = 0; i < Hd; ++i) acc += a.w2_t[i * E + o] * v1[i];
        a.ce[(long)b * E + o] = acc;
    }
}
hipError_t launch_cond_base(const CondBaseArgs& a, hipStream_t s) {
    if (a.E > 256 || a.Hd > 256) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cond_base_kernel, dim3(a.B), dim3(128), 0, s, a);
    return hipGetLastError();
}

__global__ __launch_bounds__(128) void cond_block_kernel(CondBlockArgs a) {
    __shared__ float ce[256], e[512], h1[512], red[2];
    const int b = blockIdx.x, tid = threadIdx.x, E = a.E, D = a.D;
    for (int i = tid; i < E; i += 128) ce[i] = a.ce[(long)b * E + i];
    __syncthreads();
    for (int o = tid; o < D; o += 128) {
        float acc = a.bce[o];
        for (int i = 0; i < E; ++i) acc += a.wce_t[i * D + o] * ce[i];
        e[o] = acc;
        a.emb[(long)b * D + o] = acc;
    }
    __syncthreads();
    if (tid == 0) {   // GroupNorm(1, D) over the D values of this sample (biased variance)
        float s = 0.0f;
        for (int i = 0; i < D; ++i) s += e[i];
        const float mean = s / (float)D;
        float q = 0.0f;
        for (int i = 0; i < D; ++i) { const float d = e[i] - mean; q += d * d; }
        red[0] = mean; red[1] = 1.0f / sqrtf(q / (float)D + 1e-5f);
    }
    __syncthreads();
    for (int i = tid; i < D; i += 128) e[i] = (e[i] - red[0]) * red[1] * a.gn_g[i] + a.gn_b[i];
    __syncthreads();
    for (int o = tid; o < D; o += 128) {
        float acc = a.c1_b[o];
        for (int i = 0; i < D; ++i) acc += a.c1_t[i * D + o] * e[i];
        h1[o] = act_apply(acc, ACT_GELU);
    }
    __syncthreads();
    for (int o = tid; o < D; o += 128) {
        float acc = a.c3_b[o];
        for (int i = 0; i < D; ++i) acc += a.c3_t[i * D + o] * h1[i];
        a.mul[(long)b * D + o] = 1.0f + acc;
    }
}
hipError_t launch_cond_block(const CondBlockArgs& a, hipStream_t s) {
    if (a.E > 256 || a.D > 512) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cond_block_kernel, dim3(a.B), dim3(128), 0, s, a);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void apply_kernel(ApplyArgs a) {
    const int c = blockIdx.x, b = blockIdx.y;
    const float sc = a.ss ? a.ss[((long)b * a.C + c) * 2] : 1.0f;
    const float sh = a.ss ? a.ss[((long)b * a.C + c) * 2 + 1] : 0.0f;
    const float* xs = a.x + (long)b * a.x_bs + (long)c * a.HW;
    float* ys = a.y + ((long)b * a.C + c) * a.HW;
    unsigned am = 0u;
    for (int i = threadIdx.x; i < a.HW; i += 256) {
        const float v = act_apply(xs[i] * sc + sh, a.act);
        ys[i] = v;
        am = max(am, abs_bits(v));
    }
    if (a.amax_out) { __shared__ unsigned red4[4]; amax_publish_block(a.amax_out, b, am, red4); }
}
hipError_t launch_apply(const ApplyArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(apply_kernel, dim3(a.C, a.B), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ===========================================================================
// Spectral convolution with mode truncation (FNO layer) as dense truncated DFTs.
// modules/basics.py:126-149 ; conditional scaling modules/fourier_cond.py:55-81.
// Twiddles are evaluated with sincospif on exact rational arguments ((k*n) mod N)/N.
// ===========================================================================
__device__ __forceinline__ void twiddle(int k, int n, int N, float sign, float& c, float& s) {
    const int r = (int)(((long)k * n) % N);
    sincospif(2.0f * (float)r / (float)N, &s, &c);
    s *= sign;
}
// A: t1[b,c,y,k2] = sum_x x[b,c,y,x] e^{-2 pi i k2 x / W}
__global__ __launch_bounds__(256) void spec_rows_fwd(SpectralArgs a) {
    const long n = (long)a.B * a.Cin * a.H * a.m2;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int k2 = (int)(i % a.m2);
        long r = i / a.m2;
        const int y = (int)(r % a.H); r /= a.H;
        const int c = (int)(r % a.Cin);
        const int b = (int)(r / a.Cin);
        const float* xr = a.x + (long)b * a.x_bs + ((long)c * a.H + y) * a.W;
        float re = 0.0f, im = 0.0f;
        for (int x = 0; x < a.W; ++x) {
            float cs, sn;
            twiddle(k2, x, a.W, -1.0f, cs, sn);
            re += xr[x] * cs; im += xr[x] * sn;
        }
        a.t1[i * 2] = re; a.t1[i * 2 + 1] = im;
    }
}
// B: xf[b,c,kk,k2] = sum_y t1[b,c,y,k2] e^{-2 pi i k1 y / H},  k1 = kk (kk < m1) or H - 2 m1 + kk
__global__ __launch_bounds__(256) void spec_cols_fwd(SpectralArgs a) {
    const int M1 = 2 * a.m1;
    const long n = (long)a.B * a.Cin * M1 * a.m2;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int k2 = (int)(i % a.m2);
        long r = i / a.m2;
        const int kk = (int)(r % M1); r /= M1;
        const int k1 = kk < a.m1 ? kk : a.H - M1 + kk;
        const float* tp = a.t1 + (r * a.H * a.m2 + k2) * 2;
        float re = 0.0f, im = 0.0f;
        for (int y = 0; y < a.H; ++y) {
            float cs, sn;
            twiddle(k1, y, a.H, -1.0f, cs, sn);
            const float tr = tp[(long)y * a.m2 * 2], ti = tp[(long)y * a.m2 * 2 + 1];
            re += tr * cs - ti * sn; im += tr * sn + ti * cs;
        }
        a.xf[i * 2] = re; a.xf[i * 2 + 1] = im;
    }
}
// C: of[b,o,kk,k2] = sum_i (xf[b,i,kk,k2] * emb[b]) * w[i,o,kk mod m1,k2]
__global__ __launch_bounds__(256) void spec_mix(SpectralArgs a) {
    const int M1 = 2 * a.m1;
    const long n = (long)a.B * a.Cout * M1 * a.m2;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int k2 = (int)(i % a.m2);
        long r = i / a.m2;
        const int kk = (int)(r % M1); r /= M1;
        const int o = (int)(r % a.Cout);
        const int b = (int)(r / a.Cout);
        const int hi = kk >= a.m1 ? 1 : 0, k1 = kk - hi * a.m1;
        const float* w = hi ? a.w2 : a.w1;
        float er = 1.0f, ei = 0.0f;
        if (a.emb) {
            const float* e = a.emb + ((((long)b * a.m1 + k1) * a.m2 + k2) * 2 + hi) * 2;   // [.., lo|hi, re|im]
            er = e[0]; ei = e[1];
        }
        float re = 0.0f, im = 0.0f;
        for (int c = 0; c < a.Cin; ++c) {
            const float* xp = a.xf + ((((long)b * a.Cin + c) * M1 + kk) * a.m2 + k2) * 2;
            const float xr = xp[0] * er - xp[1] * ei, xi = xp[0] * ei + xp[1] * er;
            const float* wp = w + ((((long)c * a.Cout + o) * a.m1 + k1) * a.m2 + k2) * 2;
            re += xr * wp[0] - xi * wp[1]; im += xr * wp[1] + xi * wp[0];
        }
        a.of[i * 2] = re; a.of[i * 2 + 1] = im;
    }
}
// D: t1[b,o,y,k2] = sum_kk of[b,o,kk,k2] e^{+2 pi i k1 y / H}
__global__ __launch_bounds__(256) void spec_cols_inv(SpectralArgs a) {
    const int M1 = 2 * a.m1;
    const long n = (long)a.B * a.Cout * a.H * a.m2;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int k2 = (int)(i % a.m2);
        long r = i / a.m2;
        const int y = (int)(r % a.H); r /= a.H;
        const float* op = a.of + (r * M1 * a.m2 + k2) * 2;
        float re = 0.0f, im = 0.0f;
        for (int kk = 0; kk < M1; ++kk) {
            const int k1 = kk < a.m1 ? kk : a.H - M1 + kk;
            float cs, sn;
            twiddle(k1, y, a.H, 1.0f, cs, sn);
            const float tr = op[(long)kk * a.m2 * 2], ti = op[(long)kk * a.m2 * 2 + 1];
            re += tr * cs - ti * sn; im += tr * sn + ti * cs;
        }
        a.t1[i * 2] = re; a.t1[i * 2 + 1] = im;
    }
}
// E: y[b,o,y,x] = 1/(HW) sum_k2 c_k2 Re(t1[b,o,y,k2] e^{+2 pi i k2 x / W}),  c = 1 for DC / Nyquist else 2
__global__ __launch_bounds__(256) void spec_rows_inv(SpectralArgs a) {
    const long n = (long)a.B * a.Cout * a.H * a.W;
    const float inv = 1.0f / (float)(a.H * a.W);
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int x = (int)(i % a.W);
        const long r = i / a.W;   // (b*Cout + o)*H + y
        const float* tp = a.t1 + r * a.m2 * 2;
        float acc = 0.0f;
        for (int k2 = 0; k2 < a.m2; ++k2) {
            float cs, sn;
            twiddle(k2, x, a.W, 1.0f, cs, sn);
            const float wgt = (k2 == 0 || 2 * k2 == a.W) ? 1.0f : 2.0f;
            acc += wgt * (tp[k2 * 2] * cs - tp[k2 * 2 + 1] * sn);
        }
        a.y[i] = acc * inv;
    }
}
hipError_t launch_spectral(const SpectralArgs& a, hipStream_t s) {
    if (2 * a.m1 > a.H || a.m2 > a.W / 2 + 1) return hipErrorInvalidValue;
    auto grid = [](long n) { long g = (n + 255) / 256; return dim3((unsigned)(g > 8192 ? 8192 : (g < 1 ? 1 : g))); };
    hipLaunchKernelGGL(spec_rows_fwd, grid((long)a.B * a.Cin * a.H * a.m2), dim3(256), 0, s, a);
    hipLaunchKernelGGL(spec_cols_fwd, grid((long)a.B * a.Cin * 2 * a.m1 * a.m2), dim3(256), 0, s, a);
    hipLaunchKernelGGL(spec_mix, grid((long)a.B * a.Cout * 2 * a.m1 * a.m2), dim3(256), 0, s, a);
    hipLaunchKernelGGL(spec_cols_inv, grid((long)a.B * a.Cout * a.H * a.m2), dim3(256), 0, s, a);
    hipLaunchKernelGGL(spec_rows_inv, grid((long)a.B * a.Cout * a.H * a.W), dim3(256), 0, s, a);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void fourier_combine_kernel(FourierCombineArgs a) {
    const int c = blockIdx.x, b = blockIdx.y;
    const long base = ((long)b * a.C + c) * a.HW;
    const float e = a.e ? a.e[(long)b * a.C + c] : 0.0f;
    const float* sk = a.skip ? a.skip + (long)b * a.skip_bs + (long)c * a.HW : nullptr;
    float* ys = a.y + (long)b * a.y_bs + (long)c * a.HW;
    const int act = a.act ? a.act : ACT_GELU;
    unsigned am = 0u;
    for (int i = threadIdx.x; i < a.HW; i += 256) {
        const float v = (sk ? sk[i] : 0.0f) + act_apply(a.a[base + i] + a.b[base + i] + e, act);
        ys[i] = v;
        am = max(am, abs_bits(v));
    }
    if (a.amax_out) { __shared__ unsigned red4[4]; amax_publish_block(a.amax_out, b, am, red4); }
}
hipError_t launch_fourier_combine(const FourierCombineArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(fourier_combine_kernel, dim3(a.C, a.B), dim3(256), 0, s, a);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void vec_linear_kernel(VecLinearArgs a) {
    const int b = blockIdx.y;
    for (int o = blockIdx.x * 256 + threadIdx.x; o < a.Out; o += gridDim.x * 256) {
        float acc = a.bias ? a.bias[o] : 0.0f;
        for (int i = 0; i < a.In; ++i) acc += a.in[(long)b * a.In + i] * a.w[(long)i * a.ldo + (long)o * a.ldi];
        a.out[(long)b * a.Out + o] = acc;
    }
}
hipError_t launch_vec_linear(const VecLinearArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(vec_linear_kernel, dim3((a.Out + 255) / 256, a.B), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ===========================================================================
// ===========================================================================
// Fused denormalise + relative-L2 metric (the step after the path).  HBM-bound: one read of both
// rollouts.  One block per (b, t, c) plane -> (sum of squared denormalised error, sum of squared denormalised
// truth); a second tiny kernel forms the frame-wise and sequence-wise ratios.  Fixed reduction order.
// ===========================================================================
// The per-plane body, shared by the whole-rollout kernels and the group-scoring kernel of the streaming evaluation
// (one definition: the latter must produce the former's bits).  kVecA: the prediction plane is 16-byte aligned (float4
// loads); without it the same four elements are loaded one by one and summed in the same order.  n4: float4 groups of
// the plane that are summed in the vector order (0 when the truth plane is not 16-byte aligned), the rest in element order.
template <bool kVecA>
__device__ __forceinline__ void metric_plane_sums(const float* a, const float* g, int HW, int n4, float mean, float sd,
                                                  float& d2, float& g2) {
    for (int i = threadIdx.x; i < n4; i += 256) {
        float4 p;
        if (kVecA) p = reinterpret_cast<const float4*>(a)[i];
        else p = make_float4(a[4 * i], a[4 * i + 1], a[4 * i + 2], a[4 * i + 3]);
        const float4 q = reinterpret_cast<const float4*>(g)[i];
        const float e0 = (p.x - q.x) * sd, e1 = (p.y - q.y) * sd, e2 = (p.z - q.z) * sd, e3 = (p.w - q.w) * sd;
        const float t0 = q.x * sd + mean, t1 = q.y * sd + mean, t2 = q.z * sd + mean, t3 = q.w * sd + mean;
        d2 += (e0 * e0 + e1 * e1) + (e2 * e2 + e3 * e3);
        g2 += (t0 * t0 + t1 * t1) + (t2 * t2 + t3 * t3);
    }
    for (int i = n4 * 4 + threadIdx.x; i < HW; i += 256) {
        const float e = (a[i] - g[i]) * sd, t = g[i] * sd + mean;
        d2 += e * e; g2 += t * t;
    }
}

// Per-channel statistics and the two-phase dataset's boundary handling (dataset/twophase_flow_stage2.py:370-390,
// dataset/Stage2_SW.py:60-72): v = x*std[c] + mean[c]; flag 1: the four wall rows/columns are set to zero;
// flag 2: v is clamped to [lo, hi].  Both tensors go through the same map, as the reference denormalises both.
__device__ __forceinline__ void metric_plane_ch_sums(const float* a, const float* g, int c, int H, int W,
                                                     const MetricChannelSpec& spec, float& d2, float& g2) {
    const float sd = spec.std[c], mean = spec.mean[c];
    const bool walls = spec.flags[c] & 1, clampv = spec.flags[c] & 2;
    const int HW = H * W;
    for (int i = threadIdx.x; i < HW; i += 256) {
        const int r = i / W, col = i - r * W;
        float p = a[i] * sd + mean, q = g[i] * sd + mean;
        if (walls && (r == 0 || r == H - 1 || col == 0 || col == W - 1)) { p = 0.0f; q = 0.0f; }
        if (clampv) { p = fminf(fmaxf(p, spec.lo), spec.hi); q = fminf(fmaxf(q, spec.lo), spec.hi); }
        const float e = p - q;
        d2 += e * e; g2 += q * q;
    }
}

// thread sums -> the plane's pair: wave sums, then the fixed four-wave sum (red: 8 floats of LDS)
__device__ __forceinline__ void metric_plane_store(float d2, float g2, float* red, float* out2) {
    d2 = wave_sum(d2); g2 = wave_sum(g2);
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = d2; red[4 + (threadIdx.x >> 6)] = g2; }
    __syncthreads();
    if (threadIdx.x == 0) {
        out2[0] = (red[0] + red[1]) + (red[2] + red[3]);
        out2[1] = (red[4] + red[5]) + (red[6] + red[7]);
    }
}

__global__ __launch_bounds__(256) void metric_plane_kernel(const float* yhat, const float* y, int HW, float mean, float sd,
                                                           float* part) {
    __shared__ float red[8];
    const long plane = blockIdx.x;
    const float* a = yhat + plane * HW;
    const float* g = y + plane * HW;
    float d2 = 0.0f, g2 = 0.0f;
    const int n4 = ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(g)) & 15) == 0 ? HW / 4 : 0;
    metric_plane_sums<true>(a, g, HW, n4, mean, sd, d2, g2);
    metric_plane_store(d2, g2, red, part + plane * 2);
}

__global__ __launch_bounds__(256) void metric_plane_ch_kernel(const float* yhat, const float* y, int C, int H, int W,
                                                              MetricChannelSpec spec, float* part) {
    __shared__ float red[8];
    const long plane = blockIdx.x;
    const int c = (int)(plane % C);
    const int HW = H * W;
    float d2 = 0.0f, g2 = 0.0f;
    metric_plane_ch_sums(yhat + plane * HW, y + plane * HW, c, H, W, spec, d2, g2);
    metric_plane_store(d2, g2, red, part + plane * 2);
}

// Streaming evaluation: the decode output of one group of steps, frames [kk][B][C][H*W] (a per-decode-stream buffer),
// against the truth planes y[b][y_t + j][c] of y [B][y_T][C][H*W]; the pair of plane (b, p_t + j, c) goes to its slot of
// part [B][p_T][C][2].  One block per plane, the bodies above: what metric_plane{,_ch}_kernel would write for the
// same plane of a stored rollout.  Every slot is written by exactly one block: no atomics, no dependence on the grouping.
__global__ __launch_bounds__(256) void metric_group_kernel(MetricGroupArgs a) {
    __shared__ float red[8];
    const int q = blockIdx.x;                          // (j * B + b) * C + c
    const int c = q % a.C, s = q / a.C, b = s % a.B, j = s / a.B;
    const int HW = a.H * a.W;
    const float* f = a.frames + (long)q * HW;
    const float* g = a.y + (((long)b * a.y_T + a.y_t + j) * a.C + c) * HW;
    float* out2 = a.part + (((long)b * a.p_T + a.p_t + j) * a.C + c) * 2;
    float d2 = 0.0f, g2 = 0.0f;
    if (a.norm.per_channel) {
        metric_plane_ch_sums(f, g, c, a.H, a.W, a.norm.spec, d2, g2);
    } else {
        // the stored rollout's plane (b, t, c) has the truth plane's offset, hence (equal base alignment) its alignment
        const int n4 = (reinterpret_cast<uintptr_t>(g) & 15) == 0 ? HW / 4 : 0;
        if ((reinterpret_cast<uintptr_t>(f) & 15) == 0) metric_plane_sums<true>(f, g, HW, n4, a.norm.mean, a.norm.sd, d2, g2);
        else metric_plane_sums<false>(f, g, HW, n4, a.norm.mean, a.norm.sd, d2, g2);
    }
    metric_plane_store(d2, g2, red, out2);
}

__global__ void metric_finish_kernel(const float* part, int B, int T, int C, float eps, float* frame_out, float* seq_out) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;      // (b, c)
    if (idx >= B * C) return;
    const int b = idx / C, c = idx - b * C;
    float sd = 0.0f, sg = 0.0f;
    for (int t = 0; t < T; ++t) {
        const long p = ((long)b * T + t) * C + c;
        const float d2 = part[p * 2], g2 = part[p * 2 + 1];
        if (frame_out) frame_out[p] = sqrtf(d2 / (g2 < eps ? eps : g2));
        sd += d2; sg += g2;
    }
    if (seq_out) seq_out[idx] = sqrtf(sd / (sg < eps ? eps : sg));
}

hipError_t launch_metric_rel_l2(const float* yhat, const float* y, int B, int T, int C, int HW, float mean, float sd, float eps,
                                float* frame_out, float* seq_out, float* scratch, hipStream_t s) {
    hipLaunchKernelGGL(metric_plane_kernel, dim3((unsigned)((long)B * T * C)), dim3(256), 0, s, yhat, y, HW, mean, sd, scratch);
    hipLaunchKernelGGL(metric_finish_kernel, dim3((B * C + 63) / 64), dim3(64), 0, s, scratch, B, T, C, eps, frame_out, seq_out);
    return hipGetLastError();
}

hipError_t launch_metric_rel_l2_ch(const float* yhat, const float* y, int B, int T, int C, int H, int W,
                                   const MetricChannelSpec& spec, float eps, float* frame_out, float* seq_out,
                                   float* scratch, hipStream_t s) {
    hipLaunchKernelGGL(metric_plane_ch_kernel, dim3((unsigned)((long)B * T * C)), dim3(256), 0, s, yhat, y, C, H, W, spec, scratch);
    hipLaunchKernelGGL(metric_finish_kernel, dim3((B * C + 63) / 64), dim3(64), 0, s, scratch, B, T, C, eps, frame_out, seq_out);
    return hipGetLastError();
}

hipError_t launch_metric_group(const MetricGroupArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(metric_group_kernel, dim3((unsigned)((long)a.kk * a.B * a.C)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_metric_finish(const float* part, int B, int T, int C, float eps, float* frame_out, float* seq_out, hipStream_t s) {
    hipLaunchKernelGGL(metric_finish_kernel, dim3((B * C + 63) / 64), dim3(64), 0, s, part, B, T, C, eps, frame_out, seq_out);
    return hipGetLastError();
}

// ---- ensemble statistics (lns_kernels.h EnsembleStatsArgs) ------------------------------------------------------------
// A thread owns four consecutive elements of one (step j, trajectory b) row and walks the M member rows twice (the
// second pass hits the cache: a block's 4 KB of every member row).  float4 accesses when every row starts on a 16-byte
// boundary (pointers, per and out_bs multiples of four floats: `vec`); otherwise, and for a tail, the same elements one
// by one.  An element's result depends on its M inputs only, in the order written in lns_kernels.h.
template <bool VEC>
__device__ __forceinline__ float4 ens_load(const float* p, int nv) {
    if (VEC) return *reinterpret_cast<const float4*>(p);
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    v.x = p[0];
    if (nv > 1) v.y = p[1];
    if (nv > 2) v.z = p[2];
    if (nv > 3) v.w = p[3];
    return v;
}
template <bool VEC>
__device__ __forceinline__ void ens_store(float* p, const float4& v, int nv) {
    if (VEC) { *reinterpret_cast<float4*>(p) = v; return; }
    p[0] = v.x;
    if (nv > 1) p[1] = v.y;
    if (nv > 2) p[2] = v.z;
    if (nv > 3) p[3] = v.w;
}

// products and sums are rounded one by one (hipcc contracts device code by default and honours this pragma): d * d must
// not be fused into the sum of squares, nor sd * sd / M into the subtraction
template <bool VEC>
__device__ __forceinline__ void ensemble_stats_body(const float* f, long per, int M, float* mean, float* var, int nv) {
#pragma clang fp contract(off)
    const float fm = (float)M;
    float4 s = ens_load<VEC>(f, nv);
#pragma unroll 4
    for (int m = 1; m < M; ++m) {
        const float4 v = ens_load<VEC>(f + (long)m * per, nv);
        s.x = s.x + v.x; s.y = s.y + v.y; s.z = s.z + v.z; s.w = s.w + v.w;
    }
    const float4 mu = make_float4(s.x / fm, s.y / fm, s.z / fm, s.w / fm);
    ens_store<VEC>(mean, mu, nv);
    if (!var) return;
    float4 sd = make_float4(0.0f, 0.0f, 0.0f, 0.0f), q = sd;
#pragma unroll 4
    for (int m = 0; m < M; ++m) {
        const float4 v = ens_load<VEC>(f + (long)m * per, nv);
        const float dx = v.x - mu.x, dy = v.y - mu.y, dz = v.z - mu.z, dw = v.w - mu.w;
        const float px = dx * dx, py = dy * dy, pz = dz * dz, pw = dw * dw;
        sd.x = sd.x + dx; sd.y = sd.y + dy; sd.z = sd.z + dz; sd.w = sd.w + dw;
        q.x = q.x + px; q.y = q.y + py; q.z = q.z + pz; q.w = q.w + pw;
    }
    const float fm1 = (float)(M - 1);
    float4 r;
    { const float c = sd.x * sd.x; const float k = c / fm; const float n = q.x - k; r.x = n / fm1; }
    { const float c = sd.y * sd.y; const float k = c / fm; const float n = q.y - k; r.y = n / fm1; }
    { const float c = sd.z * sd.z; const float k = c / fm; const float n = q.z - k; r.z = n / fm1; }
    { const float c = sd.w * sd.w; const float k = c / fm; const float n = q.w - k; r.w = n / fm1; }
    ens_store<VEC>(var, r, nv);
}

__global__ __launch_bounds__(256) void ensemble_stats_kernel(EnsembleStatsArgs a, int vec) {
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= a.per) return;
    const int b = blockIdx.y, j = blockIdx.z;
    const float* f = a.frames + ((long)j * a.B + b) * a.M * a.per + i;
    const long o = (long)b * a.out_bs + (long)j * a.per + i;
    const int nv = a.per - i < 4 ? (int)(a.per - i) : 4;
    if (vec && nv == 4) ensemble_stats_body<true>(f, a.per, a.M, a.mean + o, a.var ? a.var + o : nullptr, nv);
    else ensemble_stats_body<false>(f, a.per, a.M, a.mean + o, a.var ? a.var + o : nullptr, nv);
}

hipError_t launch_ensemble_stats(const EnsembleStatsArgs& a, hipStream_t s) {
    const int vec = ((reinterpret_cast<uintptr_t>(a.frames) | reinterpret_cast<uintptr_t>(a.mean) | reinterpret_cast<uintptr_t>(a.var)) & 15) == 0 &&
                    a.per % 4 == 0 && a.out_bs % 4 == 0;
    hipLaunchKernelGGL(ensemble_stats_kernel, dim3((unsigned)((a.per + 1023) / 1024), a.B, a.kk), dim3(256), 0, s, a, vec);
    return hipGetLastError();
}

// ---- ensemble validation (lns_kernels.h EnsembleScoreArgs; the statement: include/lns.h) -----------------------------
// One block per plane.  A pixel needs its M denormalised member values three times (the mean, the deviations, the pair
// sum), and M is a run-time value: a thread keeps them in its own LDS column col[m * 256 + tid] (lane-strided dwords:
// no bank conflict; nobody else reads or writes the column, so the pixel loop has no barrier).  The pair sum is
// M (M - 1) / 2 LDS reads per pixel.  Every product and sum is rounded on its own (fp contract off, as ensemble_stats_body).
__device__ __forceinline__ float score_denorm(float x, float sd, float mean, bool zero, bool clampv, float lo, float hi) {
#pragma clang fp contract(off)
    const float p = x * sd;
    float v = p + mean;
    if (zero) v = 0.0f;
    if (clampv) v = fminf(fmaxf(v, lo), hi);
    return v;
}

// Channel c of a ScoreNorm as score_denorm takes it: the scalar form has neither walls nor a clamp.  The one place the
// scored kernels (this file, spectrum.inc, field_stats.inc, time_maps.inc) unpack the rule; which pixels lie on a wall
// (`zero`) is the caller's geometry.
struct ChannelNorm {
    float sd, mean, lo, hi;
    bool walls, clampv;
    __device__ __forceinline__ ChannelNorm(const ScoreNorm& n, int c) {
        const bool pc = n.per_channel;
        sd = pc ? n.spec.std[c] : n.sd; mean = pc ? n.spec.mean[c] : n.mean; lo = n.spec.lo; hi = n.spec.hi;
        walls = pc && (n.spec.flags[c] & 1); clampv = pc && (n.spec.flags[c] & 2);
    }
};

__global__ __launch_bounds__(256) void ensemble_score_kernel(EnsembleScoreArgs a) {
#pragma clang fp contract(off)
    // all LDS is dynamic (a kernel with static LDS cannot be granted the full 160 KB of dynamic LDS init_kernels asks for):
    // [M][256] columns | red[16] | hist[M + 1]
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* red = reinterpret_cast<float*>(smem) + a.M * 256;
    int* hist = reinterpret_cast<int*>(red + 16);
    const int tid = threadIdx.x;
    const int q = blockIdx.x;                          // (j * B + b) * C + c
    const int c = q % a.C, s = q / a.C, b = s % a.B, j = s / a.B;
    const int HW = a.H * a.W, M = a.M;
    const long mstride = (long)a.C * HW;               // member to member inside frames [kk][B][M][C][HW]
    const float* f = a.frames + ((long)s * M * a.C + c) * HW;
    const long plane = ((long)b * a.y_T + a.y_t + j) * a.C + c;
    const float* g = a.y + plane * HW;
    const auto [sd, mean, lo, hi, walls, clampv] = ChannelNorm(a.norm, c);
    const float fm = (float)M, fm1 = (float)(M - 1), fpairs = (float)(M * (M - 1));
    float* col = reinterpret_cast<float*>(smem) + tid;
    for (int k = tid; k <= M; k += 256) hist[k] = 0;
    __syncthreads();
    float se_sum = 0.0f, g_sum = 0.0f, v_sum = 0.0f, cr_sum = 0.0f;
    for (int i = tid; i < HW; i += 256) {
        bool zero = false;
        if (walls) { const int r = i / a.W, cx = i - r * a.W; zero = r == 0 || r == a.H - 1 || cx == 0 || cx == a.W - 1; }
        const float qv = score_denorm(g[i], sd, mean, zero, clampv, lo, hi);
        float v = score_denorm(f[i], sd, mean, zero, clampv, lo, hi);
        col[0] = v;
        float sum = v;
#pragma unroll 4
        for (int m = 1; m < M; ++m) {
            v = score_denorm(f[m * mstride + i], sd, mean, zero, clampv, lo, hi);
            col[m * 256] = v;
            sum = sum + v;
        }
        const float mu = sum / fm;
        float dsum = 0.0f, qq = 0.0f, ab = 0.0f;
        int rank = 0;
#pragma unroll 4
        for (int m = 0; m < M; ++m) {
            v = col[m * 256];
            const float d = v - mu;
            const float p = d * d;
            dsum = dsum + d;
            qq = qq + p;
            ab = ab + fabsf(v - qv);
            rank += v < qv ? 1 : 0;
        }
        float var;
        { const float cc = dsum * dsum; const float k = cc / fm; const float n = qq - k; var = n / fm1; }
        float w = 0.0f;
        for (int m = 0; m < M - 1; ++m) {
            const float vm = col[m * 256];
#pragma unroll 4
            for (int n = m + 1; n < M; ++n) w = w + fabsf(vm - col[n * 256]);
        }
        const float t0 = ab / fm, t1 = w / fpairs;
        const float crps = t0 - t1;
        const float e = mu - qv;
        const float se = e * e, gg = qv * qv;
        se_sum = se_sum + se; g_sum = g_sum + gg; v_sum = v_sum + var; cr_sum = cr_sum + crps;
        if (a.rank) atomicAdd(&hist[rank], 1);
        if (a.pixel) {
            float* px = a.pixel + ((long)q * HW + i) * 4;
            px[0] = mu; px[1] = var; px[2] = crps; px[3] = (float)rank;
        }
    }
    se_sum = wave_sum(se_sum); g_sum = wave_sum(g_sum); v_sum = wave_sum(v_sum); cr_sum = wave_sum(cr_sum);
    if ((tid & 63) == 0) {
        const int wv = tid >> 6;
        red[wv] = se_sum; red[4 + wv] = g_sum; red[8 + wv] = v_sum; red[12 + wv] = cr_sum;
    }
    __syncthreads();
    if (tid < 4) a.scores[plane * 4 + tid] = (red[4 * tid] + red[4 * tid + 1]) + (red[4 * tid + 2] + red[4 * tid + 3]);
    if (a.rank)
        for (int k = tid; k <= M; k += 256) a.rank[plane * (M + 1) + k] = hist[k];
}

// (b, c) per thread: the four plane sums of every step -> the four scores in place; the sequence-wise forms from the
// running sums over the steps in ascending order
__global__ void ensemble_score_finish_kernel(float* scores, int B, int T, int C, int HW, float eps, float* seq) {
#pragma clang fp contract(off)
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * C) return;
    const int b = idx / C, c = idx - b * C;
    const float fhw = (float)HW, fall = (float)((long)T * HW);
    float sse = 0.0f, sg = 0.0f, sv = 0.0f, scr = 0.0f;
    for (int t = 0; t < T; ++t) {
        float* p = scores + (((long)b * T + t) * C + c) * 4;
        const float se = p[0], g2 = p[1], v = p[2], cr = p[3];
        p[0] = sqrtf(se / (g2 < eps ? eps : g2));
        p[1] = sqrtf(se / fhw);
        p[2] = sqrtf(v / fhw);
        p[3] = cr / fhw;
        sse = sse + se; sg = sg + g2; sv = sv + v; scr = scr + cr;
    }
    if (seq) {
        float* p = seq + (long)idx * 4;
        p[0] = sqrtf(sse / (sg < eps ? eps : sg));
        p[1] = sqrtf(sse / fall);
        p[2] = sqrtf(sv / fall);
        p[3] = scr / fall;
    }
}

hipError_t launch_ensemble_score(const EnsembleScoreArgs& a, hipStream_t s) {
    if (a.M < 2 || a.M > LNS_SCORE_MAX_MEMBERS) return hipErrorInvalidValue;
    const size_t lds = (size_t)a.M * 1024 + (16 + a.M + 1) * 4;            // columns, red, hist: at most 128.6 KB
    hipLaunchKernelGGL(ensemble_score_kernel, dim3((unsigned)((long)a.kk * a.B * a.C)), dim3(256), lds, s, a);
    return hipGetLastError();
}

hipError_t launch_ensemble_score_finish(float* scores, int B, int T, int C, int HW, float eps, float* seq, hipStream_t s) {
    hipLaunchKernelGGL(ensemble_score_finish_kernel, dim3((B * C + 63) / 64), dim3(64), 0, s, scores, B, T, C, HW, eps, seq);
    return hipGetLastError();
}

#include "spectrum.inc"
#include "field_stats.inc"
#include "flow_stats.inc"
#include "time_maps.inc"
#include "eval_attrib.inc"
#include "ensemble_quantile.inc"
#include "ensemble_exceed.inc"
#include "ensemble_etkf.inc"
#include "ensemble_letkf.inc"

// per-sample max |x| of a [B, n] tensor: grid (chunks, B); one atomic per wave
__global__ __launch_bounds__(256) void amax_kernel(const float* x, long x_bs, long n, unsigned* amax) {
    const int b = blockIdx.y;
    const float* xs = x + (long)b * x_bs;
    unsigned am = 0u;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) am = max(am, abs_bits(xs[i]));
    __shared__ unsigned red4[4];
    amax_publish_block(amax, b, am, red4);
}
hipError_t launch_amax(const float* x, long x_bs, long n, int B, unsigned* amax, hipStream_t s) {
    long chunks = (n + 256 * 16 - 1) / (256 * 16);
    chunks = chunks < 1 ? 1 : (chunks > 256 ? 256 : chunks);
    hipLaunchKernelGGL(amax_kernel, dim3((unsigned)chunks, B), dim3(256), 0, s, x, x_bs, n, amax);
    return hipGetLastError();
}

// OR "some amax word of the region holds a non-finite bit pattern" into *flag (lns_check_finite's memory of the runs
// whose amax region has been zeroed again since); launched in front of the region's memset when tracking is on
__global__ __launch_bounds__(256) void amax_sticky_kernel(const unsigned* amax, int n, unsigned* flag) {
    bool bad = false;
    for (int i = threadIdx.x; i < n; i += 256) bad = bad || ((amax[i] >> 23) & 0xffu) == 0xffu;
    if (__builtin_amdgcn_ballot_w64(bad) != 0ull && (threadIdx.x & 63) == 0) atomicOr(flag, 1u);
}
hipError_t launch_amax_sticky(const unsigned* amax, int n, unsigned* flag, hipStream_t s) {
    hipLaunchKernelGGL(amax_sticky_kernel, dim3(1), dim3(256), 0, s, amax, n, flag);
    return hipGetLastError();
}

// an empty launch: calibration of the per-launch overhead of the engine's HIP-event timing (Runner::finish)
__global__ void empty_kernel() {}
hipError_t launch_empty(hipStream_t s) {
    hipLaunchKernelGGL(empty_kernel, dim3(1), dim3(64), 0, s);
    return hipGetLastError();
}

hipError_t init_kernels() {
    hipError_t e;
    const int maxlds = 160 * 1024;
#define LNS_SET_LDS(k)                                                                            \
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, maxlds); \
    if (e != hipSuccess) return e;
    LNS_SET_LDS(conv3_up2d_kernel)
#ifdef LNS_EXPERIMENTAL
    LNS_SET_LDS((conv3_up2q_kernel<true>))
    LNS_SET_LDS((conv3_up2q_kernel<false>))
    LNS_SET_LDS(conv3_w8_kernel<1>)
    LNS_SET_LDS(conv3_w8_kernel<2>)
    LNS_SET_LDS((conv3_up2r_kernel<true>))
    LNS_SET_LDS((conv3_up2r_kernel<false>))
    LNS_SET_LDS((conv3_pc_kernel<1, 1>))
    LNS_SET_LDS((conv3_pc_kernel<1, 2>))
    LNS_SET_LDS((conv3_pc_kernel<2, 1>))
    LNS_SET_LDS((conv3_pc_kernel<2, 2>))
#endif
    LNS_SET_LDS((conv_mfma_kernel<2, 4, 2, 2, 3, false, 4>))
    LNS_SET_LDS((conv_mfma_kernel<2, 4, 2, 2, 3, false, 8>))
    LNS_SET_LDS((conv_mfma_kernel<2, 4, 2, 2, 1, true, 16>))
    LNS_SET_LDS((conv_mfma_kernel<2, 4, 2, 2, 1, false, 16>))
    LNS_SET_LDS((conv_mfma_kernel<2, 2, 1, 4, 3, false, 4>))
    LNS_SET_LDS((conv_mfma_kernel<2, 2, 1, 4, 3, false, 4, true>))
    LNS_SET_LDS((conv_mfma_kernel<2, 2, 1, 4, 3, false, 8, true>))
    LNS_SET_LDS((conv_mfma_kernel<2, 2, 1, 4, 1, true, 16, true>))
    LNS_SET_LDS((conv_mfma_kernel<2, 2, 1, 4, 1, false, 16, true>))
    LNS_SET_LDS((conv_mfma_kernel<2, 2, 1, 4, 3, false, 8>))
    LNS_SET_LDS((conv_mfma_kernel<2, 2, 1, 4, 1, true, 16>))
    LNS_SET_LDS((conv_mfma_kernel<2, 2, 1, 4, 1, false, 16>))
    LNS_SET_LDS((conv_mfma_kernel<2, 2, 2, 2, 3, false, 4>))
    LNS_SET_LDS((conv_mfma_kernel<2, 2, 2, 2, 3, false, 8>))
    LNS_SET_LDS((conv_mfma_kernel<2, 2, 2, 2, 1, true, 16>))
    LNS_SET_LDS((conv_mfma_kernel<2, 2, 2, 2, 1, false, 16>))
    LNS_SET_LDS((conv_mfma_kernel<2, 1, 1, 4, 3, false, 4>))
    LNS_SET_LDS((conv_mfma_kernel<2, 1, 1, 4, 3, false, 4, true>))
    LNS_SET_LDS((conv_mfma_kernel<2, 1, 1, 4, 3, false, 8, true>))
    LNS_SET_LDS((conv_mfma_kernel<2, 1, 1, 4, 1, true, 16, true>))
    LNS_SET_LDS((conv_mfma_kernel<2, 1, 1, 4, 1, false, 16, true>))
    LNS_SET_LDS((conv_mfma_kernel<2, 1, 1, 4, 3, false, 8>))
    LNS_SET_LDS((conv_mfma_kernel<2, 1, 1, 4, 1, true, 16>))
    LNS_SET_LDS((conv_mfma_kernel<2, 1, 1, 4, 1, false, 16>))
    LNS_SET_LDS((conv_mfma_kernel<1, 1, 2, 2, 3, false, 4>))
    LNS_SET_LDS((conv_mfma_kernel<1, 1, 2, 2, 3, false, 8>))
    LNS_SET_LDS((conv_mfma_kernel<1, 1, 2, 2, 1, true, 16>))
    LNS_SET_LDS((conv_mfma_kernel<1, 1, 2, 2, 1, false, 16>))
    LNS_SET_LDS((conv_mfma_kernel<1, 1, 1, 4, 3, false, 4>))
    LNS_SET_LDS((conv_mfma_kernel<1, 1, 1, 4, 3, false, 8>))
    LNS_SET_LDS((conv_mfma_kernel<1, 1, 1, 4, 1, true, 16>))
    LNS_SET_LDS((conv_mfma_kernel<1, 1, 1, 4, 1, false, 16>))
    LNS_SET_LDS(spectrum_group_kernel)
    LNS_SET_LDS(spectrum_stored_kernel)
#define LNS_SET_SWB(HT, WT)                                                                                              \
    {                                                                                                                    \
        constexpr int NWV = fa_sandwich_b_lds_const(HT, WT, 4) <= 160 * 1024 ? 4 : 3;                                    \
        constexpr bool UL = HT * WT >= 6;                                                                                \
        LNS_SET_LDS((fa_sandwich_b_kernel<HT, WT, true, (HT == WT), NWV, UL>))                                           \
        LNS_SET_LDS((fa_sandwich_b_kernel<HT, WT, true, false, NWV, UL>))                                                \
        LNS_SET_LDS((fa_sandwich_b_kernel<HT, WT, false, false, NWV, UL>))                                               \
    }
    LNS_SET_SWB(1, 1) LNS_SET_SWB(1, 2) LNS_SET_SWB(2, 1) LNS_SET_SWB(2, 2) LNS_SET_SWB(2, 3)
#undef LNS_SET_SWB
#define LNS_SET_SWF(HT, WT)                                                                                              \
    {                                                                                                                    \
        constexpr bool ULF = false;                                                                                      \
        LNS_SET_LDS((fa_sandwich_f_kernel<HT, WT, true, (HT == WT), ULF>))                                               \
        LNS_SET_LDS((fa_sandwich_f_kernel<HT, WT, true, false, ULF>))                                                    \
        LNS_SET_LDS((fa_sandwich_f_kernel<HT, WT, false, false, ULF>))                                                   \
    }
    LNS_SET_SWF(1, 1) LNS_SET_SWF(1, 2) LNS_SET_SWF(2, 1) LNS_SET_SWF(2, 2) LNS_SET_SWF(2, 3)
#undef LNS_SET_SWF
    LNS_SET_LDS((fa_fused_kernel<2>))
    LNS_SET_LDS((fa_fused2_kernel<2>))
    LNS_SET_LDS((fa_fused_g_kernel<2, 2, 2>))
    LNS_SET_LDS((fa_fused_g_kernel<4, 1, 1>))
    LNS_SET_LDS((fa_fused_g_kernel<2, 1, 1>))
    LNS_SET_LDS((fa_sandwich_kernel<1, 1, true>))
    LNS_SET_LDS((fa_sandwich_kernel<1, 1, false>))
    LNS_SET_LDS((fa_sandwich_kernel<1, 2, true>))
    LNS_SET_LDS((fa_sandwich_kernel<1, 2, false>))
    LNS_SET_LDS((fa_sandwich_kernel<2, 2, true>))
    LNS_SET_LDS((fa_sandwich_kernel<2, 2, false>))
    LNS_SET_LDS((fa_sandwich_kernel<2, 3, true>))
    LNS_SET_LDS((fa_sandwich_kernel<2, 3, false>))
    LNS_SET_LDS((fa_sandwich_kernel<2, 1, true>))
    LNS_SET_LDS((fa_sandwich_kernel<2, 1, false>))
    LNS_SET_LDS((conv1s_bf16x3_kernel<true>))
    LNS_SET_LDS((conv1s_bf16x3_kernel<false>))
    LNS_SET_LDS((conv1_bf16x3_kernel<true, true>))
    LNS_SET_LDS((conv1_bf16x3_kernel<true, false>))
    LNS_SET_LDS((conv1_bf16x3_kernel<false, true>))
    LNS_SET_LDS((conv1_bf16x3_kernel<false, false>))
    LNS_SET_LDS((conv3_bf16x3_kernel<1, 1, false, 2, 2>))
    LNS_SET_LDS((conv3_bf16x3_kernel<1, 1, false, 2, 2, 4>))
    LNS_SET_LDS((conv3_bf16x3_kernel<1, 2, false, 2, 2, 4>))
    LNS_SET_LDS((conv3_bf16x3_kernel<1, 1, true, 2, 2, 4>))
    LNS_SET_LDS((conv3_bf16x3_kernel<1, 2, true, 2, 2, 4>))
    LNS_SET_LDS((conv3_bf16x3_kernel<1, 1, false, 2, 2, 9, true>))       // OCT8-input instantiations (ConvArgs::x_oct)
    LNS_SET_LDS((conv3_bf16x3_kernel<1, 2, false, 2, 2, 9, true>))
    LNS_SET_LDS((conv3_bf16x3_kernel<1, 1, true, 2, 2, 9, true>))
    LNS_SET_LDS((conv3_bf16x3_kernel<1, 2, true, 2, 2, 9, true>))
    LNS_SET_LDS((conv3_bf16x3_kernel<1, 1, false, 2, 2, 4, true>))
    LNS_SET_LDS((conv3_bf16x3_kernel<1, 2, false, 2, 2, 4, true>))
    LNS_SET_LDS((conv3_bf16x3_kernel<1, 1, true, 2, 2, 4, true>))
    LNS_SET_LDS((conv3_bf16x3_kernel<1, 2, true, 2, 2, 4, true>))
    LNS_SET_LDS((conv3_bf16x3_kernel<1, 1, false, 1, 2, 9, true>))
    LNS_SET_LDS((conv3_bf16x3_kernel<1, 2, false, 1, 2, 9, true>))
    LNS_SET_LDS((conv3_bf16x3_kernel<2, 2, false, 2, 2>))
    LNS_SET_LDS((conv3_bf16x3_kernel<2, 2, true, 2, 2>))
    LNS_SET_LDS((conv3_bf16x3_kernel<1, 2, false, 2, 2>))
    LNS_SET_LDS((conv3_bf16x3_kernel<1, 1, true, 2, 2>))
    LNS_SET_LDS((conv3_bf16x3_kernel<1, 2, true, 2, 2>))
    LNS_SET_LDS((conv3_bf16x3_kernel<1, 1, false, 1>))
    LNS_SET_LDS((conv3_bf16x3_kernel<1, 1, false, 1, 2>))
    LNS_SET_LDS((conv3_bf16x3_kernel<1, 2, false, 1, 2>))
    LNS_SET_LDS((conv3_bf16x3_kernel<1, 2, false, 1>))
    LNS_SET_LDS((conv3_bf16x3_kernel<1, 1, true>))
    LNS_SET_LDS((conv3_bf16x3_kernel<1, 1, false>))
    LNS_SET_LDS((conv3_bf16x3_kernel<1, 2, true>))
    LNS_SET_LDS((conv3_bf16x3_kernel<1, 2, false>))
    LNS_SET_LDS(fa_reducer_mfma_kernel)
    LNS_SET_LDS(fa_reducer2_mfma_kernel)
    LNS_SET_LDS(fa_lrk_kernel)
    LNS_SET_LDS(fa_lrk2_kernel)
    LNS_SET_LDS(fa_pool_kernel)
    LNS_SET_LDS(fa_reducer_kernel)
    LNS_SET_LDS(ensemble_score_kernel)                                   // 128 members: 128 KB of columns
    LNS_SET_LDS(ensemble_quantile_kernel)                                // likewise
    LNS_SET_LDS(ensemble_obs_gram_kernel<4>)                             // 64 members: 67.5 KB of anomalies
    LNS_SET_LDS(letkf_patch_gram_kernel<4>)                              // likewise
    LNS_SET_LDS(letkf_combine_kernel)                                    // 4096 domains: 144 KB of weights and the patch list
    LNS_SET_LDS(etkf_transform_kernel)                                   // 64 members: A and Q, 64 KB
    LNS_SET_LDS(ensemble_transform_kernel)                               // 64 members: 64 KB of columns and X
#undef LNS_SET_LDS
    return hipSuccess;
}

}  // namespace lns

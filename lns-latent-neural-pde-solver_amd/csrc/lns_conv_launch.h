// How a convolution launch is built on the host: padded pack sizes, tiling, source maps, the geometry part of ConvArgs, the
// fp16-split weight scale, the GroupNorm fold.  The one home of these rules: the planner, the op-level entry points, the
// training plans and the model builder all call them, so an op-level test launches a kernel with the arguments a plan would
// give it.  Host only: no HIP call, nothing that needs a device (tests/native/conv_launch_check.cpp runs it without one).
#pragma once
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/lns.h"
#include "lns_kernels.h"
#include "lns_knobs.h"

namespace lns {

// padded sizes of a conv pack [taps][Cin_pad][Cout_pad]: channel stages of 8 (3x3) or 32 (1x1), 32 / 64 / multiples of 128 couts
struct ConvPadded { int kc_log2, Cin_pad, Cout_pad; };
inline ConvPadded conv_padded_sizes(int k, int cin, int cout) {
    const int kc_log2 = k == 3 ? 3 : 5, kc = 1 << kc_log2;
    return ConvPadded{kc_log2, (cin + kc - 1) / kc * kc, cout <= 32 ? 32 : (cout <= 64 ? 64 : (cout + 127) / 128 * 128)};
}

// the power of two that brings the largest |w| of a layer just below 2^14 before its two-term fp16 split.  wmax positive and
// finite: what an all-zero or non-finite weight array packs at is each caller's own decision.
inline float conv_f16_weight_scale(float wmax) { return exp2f(floorf(log2f(16000.0f / wmax))); }
// accumulator scale of the epilogue: 1 / (weight scale) for the kernels whose slabs hold w * wscale, else 1
inline float conv_unscale(int variant, float wscale) {
    return (cv_is_f16x2_3x3(variant) || variant == CV_B1) ? 1.0f / wscale : 1.0f;
}

// legacy 'nearest': src = min(floor(dst*scale), in-1), scale = in/out in fp32 unless given
// (F.interpolate(scale_factor=2.0) basics.py:296 -> scale 0.5; nn.Upsample(size) autoencoder2d.py:134)
inline int nearest_src(int dst, int in, int out, float scale) {
    if (in == out) return dst;
    const float sc = scale > 0.0f ? scale : (float)in / (float)out;
    int s = (int)floorf((float)dst * sc);
    return s < in - 1 ? s : in - 1;
}

// padded/virtual coordinate -> source index (or -1 = zero).  `len` entries.
inline void build_axis_map(std::vector<int>& out, int len, int in, int virt, float scale, int pad_lo, int pad_hi,
                           int mode) {
    out.resize(len);
    for (int p = 0; p < len; ++p) {
        int u = p - pad_lo;
        int src = -1;
        if (p < virt + pad_lo + pad_hi) {
            if (u < 0 || u >= virt) {
                if (mode == LNS_PAD_CIRCULAR) { u %= virt; if (u < 0) u += virt; }
                else u = -1;
            }
            if (u >= 0) src = nearest_src(u, in, virt, scale);
        }
        out[p] = src;
    }
}

struct ConvGeom { int variant, bw_log2, tiles_x, tiles_y, cout_tiles, PH, PW, Hout, Wout, kc_log2, sel_kc_log2; };

inline bool conv_geometry(ConvGeom& g, int B, int Cout, int Hv, int Wv, int k, int stride, int dil, const int* pad,
                          int kc_log2_pack, int Cout_pad, int force_variant, bool need_wgm1 = false,
                          bool allow_bf16x3 = false, int Cin = 1 << 30, bool f16x2 = false, bool allow_thin = false,
                          int force_bw_log2 = -1 /* 3x3: only this tile width (the quad-phase upsampling conv wants 8 x 16 tiles) */) {
    g.Hout = (Hv + pad[0] + pad[1] - dil * (k - 1) - 1) / stride + 1;
    g.Wout = (Wv + pad[2] + pad[3] - dil * (k - 1) - 1) / stride + 1;
    if (g.Hout <= 0 || g.Wout <= 0) return false;
    std::vector<int> cands;
    if (force_variant >= 0) cands = {force_variant};
    else if (Cout <= 32) cands = {CV_S32};
    else if (Cout <= 64) cands = need_wgm1 ? std::vector<int>{CV_L64, CV_M64} : std::vector<int>{CV_L64, CV_M64, CV_S64};
    else if (knobs().conv_use_128) cands = {CV_L128, CV_M128, CV_S64};   // tuning knob (tile choice only)
    else cands = {CV_L64, CV_M64, CV_S64};   // 64-cout tiles at 2 waves/SIMD beat 128-cout tiles at 1 (measured)
    // bf16x3 kernel for every eligible 3x3 conv.  Eligibility is a function of the layer only (never of B):
    // the fp32 variants accumulate in a different order, and a trajectory must not change bitwise with the
    // batch it is computed in.
    const bool no_bf16x3 = knobs().conv_fp32_mfma;
    const bool use_b = allow_bf16x3 && !no_bf16x3 && k == 3 && stride == 1 && Cout > 32;
    if (force_variant < 0 && use_b) {   // fp32 variants only if the geometry rules the bf16x3 tiles out
        cands.insert(cands.begin(), f16x2 ? (int)CV_F64 : (int)CV_B64);
    }
    const bool no_b1 = knobs().conv1_fp32_mfma;
    // 1x1: bf16x3 unless the layer is a thin projection (few output channels / a handful of input channels:
    // bandwidth-bound, and a 64-cout MFMA tile would be mostly padding) -- again a per-layer rule
    if (force_variant < 0 && allow_bf16x3 && !no_bf16x3 && !no_b1 && k == 1 && stride == 1 && Cout > 32 && Cin >= 16)
        cands = {(int)CV_B1};
    // <= 4 output channels (the decoder's last conv): streaming VALU kernel, one HBM read of the input
    const bool no_thin = knobs().conv1_no_thin;
    if (force_variant < 0 && allow_thin && !no_thin && k == 1 && stride == 1 && Cout <= 4 && Cin <= 512 && (Hv * Wv) % 4 == 0)
        cands = {(int)CV_THIN};
    g.kc_log2 = conv_pick_kc_log2(k, stride, kc_log2_pack);
    static const int pref[] = {5, 6, 4, 7, 3, 8};   // log2 BW preference on ties: 32,64,16,128,8,256
    bool found = false;
    for (size_t ci = 0; ci < cands.size(); ++ci) {
        const ConvVariantInfo vi = conv_variant_info(cands[ci]);
        if (cands[ci] < CV_B64 && Cout_pad % vi.TM != 0) continue;   // fp32 pack layout
        ConvArgs tmp;
        memset(&tmp, 0, sizeof tmp);
        tmp.ks = k; tmp.kc_log2 = g.kc_log2; tmp.Cin_pad = 1 << kc_log2_pack;
        if (cands[ci] >= CV_B64) { tmp.stride = stride; tmp.Cin_pad = 512; tmp.wb = &tmp; }
        int best_bw = -1, txn = 0, tyn = 0, best_kc = g.kc_log2;
        if (k == 1) {
            // 1x1: the image is a flat array of H*W pixels, a tile is TN consecutive pixels
            if (stride != 1 || pad[0] || pad[1] || pad[2] || pad[3]) return false;
            tmp.PH = 1; tmp.PW = 1;
            if (!conv_fits(cands[ci], tmp)) continue;
            best_bw = 0;
            while ((1 << best_bw) < vi.TN) ++best_bw;
            txn = (g.Hout * g.Wout + vi.TN - 1) / vi.TN; tyn = 1;
        } else {
            long best_cost = -1;
            for (int pi = 0; pi < 6; ++pi) {
                const int lb = pref[pi];
                const int BW = 1 << lb;
                if (BW > vi.TN || (force_bw_log2 >= 0 && lb != force_bw_log2)) continue;
                const int BH = vi.TN / BW;
                const long cost = (long)((g.Hout + BH - 1) / BH) * BH * ((g.Wout + BW - 1) / BW) * BW;
                tmp.PH = (BH - 1) * stride + (k - 1) * dil + 1;
                tmp.PW = (BW - 1) * stride + (k - 1) * dil + 1;
                tmp.kc_log2 = g.kc_log2;
                if (!conv_fits(cands[ci], tmp)) {
                    if (cands[ci] == CV_B64) continue;
                    tmp.kc_log2 = 2;
                    if (!conv_fits(cands[ci], tmp)) continue;
                }
                if (best_cost < 0 || cost < best_cost) { best_cost = cost; best_bw = lb; best_kc = tmp.kc_log2; }
            }
            if (best_bw < 0) continue;
            const int BW = 1 << best_bw, BH = vi.TN / BW;
            txn = (g.Wout + BW - 1) / BW; tyn = (g.Hout + BH - 1) / BH;
            tmp.PH = (BH - 1) * stride + (k - 1) * dil + 1;
            tmp.PW = (BW - 1) * stride + (k - 1) * dil + 1;
        }
        const long blocks = (long)B * txn * tyn * ((Cout + vi.TM - 1) / vi.TM);
        g.variant = cands[ci]; g.bw_log2 = best_bw; g.tiles_x = txn; g.tiles_y = tyn;
        g.cout_tiles = (Cout + vi.TM - 1) / vi.TM;
        g.PH = tmp.PH; g.PW = tmp.PW; g.sel_kc_log2 = best_kc;
        found = true;
        if (cands[ci] == CV_B64 && Cout >= 64 && !need_wgm1 && force_variant < 0) {
            // 32-cout tiles (same accumulation order, same bits) when 64-cout tiles give fewer blocks than this.
            // Measured on NS2d-128 (16x16 latent layers, 256 -> 512 blocks): no gain (17.9k vs 18.7k
            // trajectory-steps/s), so the default is off; kept as a tuning knob and covered by the kernel tests.
            if (blocks < knobs().convb32_below) { g.variant = CV_B32; g.cout_tiles = (Cout + 31) / 32; }
        }
        if (cands[ci] == CV_F64 && Cout >= 64 && !need_wgm1 && force_variant < 0) {
            // the same for the f16x2 form.  On 256-block launches (the 16x16 latent layers of NS2d at B = 64) it measured
            // neutral to slower (round 1: rollout 144.3 -> 148.1 ms; round 3: 22.6 -> 22.9 us per layer -- every block still
            // stages and splits the whole patch), but launches that leave three quarters of the CUs idle gain: the 7 x 15
            // latent layers of the two-phase models at B = 32 (64 blocks) 19.7 -> 15.3 us, dilated 20.5 -> 17.8
            // (tools/conv_time.py lat_tp / lat_tp_d4, variant 13).  Same bits either way, so the batch may decide.
            if (blocks < knobs().convf32_below) { g.variant = CV_F32; g.cout_tiles = (Cout + 31) / 32; }
        }
        if (cands[ci] >= CV_B64) break;                        // never fall through to another kernel family by launch size
        if (blocks >= knobs().conv_min_blocks) break;
    }
    return found;
}

// row / column source maps of a tiling: every padded position a tile's patch can touch, (tiles - 1) * tile * stride + patch
// entries per axis.  Hv x Wv: the plane the convolution sees (the source of the phase form; a resize target otherwise).
inline void conv_tile_maps(std::vector<int>& rm, std::vector<int>& cm, const ConvGeom& g, int stride, int Hin, int Win, int Hv,
                           int Wv, float sch, float scw, const int* pad, int my, int mx) {
    const int BW = 1 << g.bw_log2, BH = conv_variant_info(g.variant).TN / BW;
    build_axis_map(rm, (g.tiles_y - 1) * BH * stride + g.PH, Hin, Hv, sch, pad[0], pad[1], my);
    build_axis_map(cm, (g.tiles_x - 1) * BW * stride + g.PW, Win, Wv, scw, pad[2], pad[3], mx);
}

// a tiling and the layer's static facts -> ConvArgs: dims, dense batch strides (a caller whose tensors are strided or
// tagged overwrites x_bs / y_bs), padded channel counts, tiles, patch and its division constant.  g.Hout x g.Wout is the
// stored plane (the phase form: twice the source, set by the caller).
inline void conv_set_geometry(ConvArgs& a, const ConvGeom& g, int B, int Cin, int Hin, int Win, int Cout, int k, int stride,
                              int dil, int Cin_pad, int Cout_pad) {
    a.Cin = Cin; a.Hin = Hin; a.Win = Win; a.x_bs = (long)Cin * Hin * Win;
    a.Cout = Cout; a.Hout = g.Hout; a.Wout = g.Wout; a.y_bs = (long)Cout * g.Hout * g.Wout;
    a.ks = k; a.stride = stride; a.dil = dil; a.Cin_pad = Cin_pad; a.Cout_pad = Cout_pad;
    // 16-byte patch loads: every channel row of every sample must start 16-byte aligned
    a.vec4 = (k == 1 && ((Hin * Win) % 4 == 0)) ? 1 : 0;
    a.kc_log2 = g.sel_kc_log2; a.tiles_x = g.tiles_x; a.tiles_y = g.tiles_y; a.cout_tiles = g.cout_tiles;
    a.bw_log2 = g.bw_log2; a.PH = g.PH; a.PW = g.PW; a.B = B;
    a.ph_magic = g.PH > 1 ? (unsigned)((0x100000000ull + g.PH - 1) / g.PH) : 0u;
}

// No resize, pads inside one period: the split-operand 3x3 kernel computes its source maps itself (ConvArgs::map_arith).
// Hv x Wv is the plane the maps were built for, AFTER the phase form's rewrite to the source size (Hv = Hin, Wv = Win).
// "No resize" is Hv == Hin && Wv == Win.  The planner used to write it as `up2 || (!in.vH && !in.vW)`; the two agree:
// a TRef's virtual size is only ever set as (2H, 2W) or as a target (outH, outW) != (H, W), both components together, so
// vH != 0 means (Hv, Wv) != (H, W) before the rewrite and vH == 0 means Hv == H && Wv == W; the phase form (up2) rewrites
// (Hv, Wv) to (H, W) on both sides.  LNS_NO_ARITH_MAPS (A/B knob): table reads everywhere.
inline void conv_set_map_arith(ConvArgs& a, int variant, int k, int Hin, int Win, int Hv, int Wv, const int* pad, int my, int mx) {
    if (knobs().no_arith_maps || k != 3 || Hv != Hin || Wv != Win || !cv_is_split_3x3(variant)) return;
    if (pad[0] > Hin || pad[1] > Hin || pad[2] > Win || pad[3] > Win) return;
    if ((my != LNS_PAD_ZEROS && my != LNS_PAD_CIRCULAR) || (mx != LNS_PAD_ZEROS && mx != LNS_PAD_CIRCULAR)) return;
    a.map_arith = 1;
    a.map_circ[0] = my == LNS_PAD_CIRCULAR; a.map_circ[1] = mx == LNS_PAD_CIRCULAR;
    a.map_pad[0] = pad[0]; a.map_pad[1] = pad[2];
    a.map_ext[0] = Hin + pad[0] + pad[1]; a.map_ext[1] = Win + pad[2] + pad[3];
}

// GroupNorm folded into a consumer's prologue: instead of a finished (scale, shift) table the consumer reads the tile
// partials its producer left (ConvArgs::stat_part of that launch) and merges them itself.  gn_count: pixels behind every
// partial as gn_tile_rule gives it (GN_TILE_PIXELS is the kernel's default, passed as 0).
inline void conv_fold_gn(ConvArgs& a, const float* part, int tiles, int gn_count, int groups, float eps, const float* premul,
                         const float* gamma, const float* beta) {
    a.ss = nullptr;
    a.gn_part = part; a.gn_tiles = tiles; a.gn_groups = groups; a.gn_eps = eps;
    a.gn_count = gn_count == GN_TILE_PIXELS ? 0 : gn_count; a.gn_premul = premul;
    a.gn_gamma = gamma; a.gn_beta = beta;
}

// bound of a GroupNorm output whatever the data, a layer constant: |(v - mean) rstd| <= sqrt(n - 1) over a group of n values
// (biased variance), so |gamma| sqrt(n_group) + |beta| bounds the normalised tensor
inline float gn_output_bound(float gamma_max, float beta_max, int ch_per_group, int H, int W) {
    return gamma_max * sqrtf((float)ch_per_group * H * W) + beta_max;
}
// ... handed to the split-operand consumer as the final bound of its transformed input: no per-sample maximum is read
inline void conv_set_final_bound(ConvArgs& a, float bound) { a.amax_in = nullptr; a.amax_in_const = bound; a.bound_final = 1; }

}  // namespace lns

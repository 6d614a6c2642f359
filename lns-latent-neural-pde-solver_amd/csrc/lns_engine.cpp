// LNS rollout engine: weight packing, launch planning, execution, C ABI.
// Replaces (behind include/lns.h) the reference's
//   LatentDynamics.predict            train_stage2_ns2d.py:143-158
//   SimpleAutoencoder.encode/decode   modules/autoencoder2d.py:174-182
//   SimpleCNN.forward                 train_stage2_ns2d.py:82-87
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <tuple>
#include <stdexcept>

#include "lns_conv_launch.h"
#include "lns_engine.h"
#include "lns_fold.h"
#include "lns_op_scratch.h"
#include "lns_resolve.h"
#include "lns_spectrum.h"

// the batch is a grid dimension (gridDim.y / .z) of every kernel
#define LNS_MAX_BATCH 65535

namespace lns {
void build_model(lns_engine* e);

static thread_local std::string g_create_error;

static std::string fmt(const char* f, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, f);
    vsnprintf(buf, sizeof buf, f, ap);
    va_end(ap);
    return buf;
}

#define HIPCHK(e, call)                                                                         \
    do {                                                                                        \
        hipError_t err__ = (call);                                                              \
        if (err__ != hipSuccess) {                                                              \
            (e)->err = fmt("%s failed: %s (%s:%d)", #call, hipGetErrorString(err__), __FILE__, __LINE__); \
            return LNS_EHIP;                                                                    \
        }                                                                                       \
    } while (0)

static size_t round_up_sz(size_t v, size_t m) { return (v + m - 1) / m * m; }

// (how the planner, the op-level entry points and training build a conv launch: lns_conv_launch.h)
// [Cout][Cin][k][k] slices -> [taps][Cin_pad][Cout_pad]
static void pack_conv_weight(float* dst, const float* src, int cout_off, int cout, int cin, int k, int Cin_pad,
                             int Cout_pad) {
    const int taps = k * k;
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci)
            for (int t = 0; t < taps; ++t)
                dst[((size_t)t * Cin_pad + ci) * Cout_pad + cout_off + co] = src[((size_t)co * cin + ci) * taps + t];
}

// ---------------------------------------------------------------------------
// GroupNorm fed by the tile statistics of the convolution that produced its input: which producers leave per-tile
// (mean, M2) partials in their epilogue (ConvArgs::stat_part), over which pixel counts, and whether the merge can be
// folded into the consumer's prologue.  One rule for Planner::emit_gn and the op-level entry point lns_op_conv_gn, so that
// the latter tests the decision itself.  Layer-static (never a function of the batch beyond the scratch capacity).
// ---------------------------------------------------------------------------
enum { GN_TILES_EXACT = 0, GN_TILES_RAGGED1 = 1, GN_TILES_RAGGEDN = 2 };
struct GnTileRule {
    int mode;              // GN_TILES_*
    int tiles;             // partials per (sample, channel); the phase form of an upsampling conv: four per source tile
    int stat_count;        // ConvArgs::stat_count of the producer: 0, H * W (one ragged tile) or -1 (ragged tiles)
    int gn_count;          // pixels behind every partial: GN_TILE_PIXELS, H * W, or -1 (unequal: `geom`)
    GnTileGeom geom;       // mode GN_TILES_RAGGEDN only
    bool foldable;         // the merge may run in a split-operand consumer's prologue (ConvArgs::gn_part)
};
// c / variant: the producing convolution as emitted; H, W: the plane the GroupNorm sees (c.Cout channels); premul: the norm
// has a per-sample channel multiplier; stat_cap: bytes of the partials scratch.  False: no tile statistics for this pair.
static bool gn_tile_rule(GnTileRule& r, const ConvArgs& c, int variant, int H, int W, int groups, bool premul, int B, size_t stat_cap) {
    // From 16 x 16 planes up (two 128-pixel tiles): below 1024 pixels the merge launch used to cost what the statistics
    // launch cost, but the merge now happens inside the consumer convolution (no launch at all) whenever it can.
    const Knobs& kn = knobs();
    const bool no_fold = kn.gn_no_fold;        // A/B knob: round 2's behaviour
    const long min_hw = kn.gn_fuse_min_hw;     // (256; 1024 under LNS_GN_NO_FOLD)
    // producers with the statistics epilogue: the split-operand 3x3 kernels and the streaming 1x1 kernel (not its
    // input-stationary form, not with a fused second conv: its statistics would be taken of the wrong tensor... they
    // are taken of what is stored, which is right -- but only the plain form is covered by tests:
    // tests/test_conv_gn_stats_gpu.py through lns_op_conv_gn)
    // Planes below 128 pixels (the 7 x 15 latents of the two-phase models) are ONE ragged tile: its epilogue takes exact
    // two-pass statistics over the valid pixels (ConvArgs::stat_count) -- the three statistics launches per conditional
    // block were a quarter of config 4's dependency chain.  A per-sample channel multiplier (premul) is applied
    // to the partials by whoever merges them.
    const bool no_ragged = kn.gn_no_ragged;
    const bool ragged1 = !no_fold && !no_ragged && !c.up2 && c.tiles_x * c.tiles_y == 1 && H * W < GN_TILE_PIXELS;
    // ... and planes whose 128-pixel tiles do not cover them exactly (14 x 30, 28 x 60, 61 x 121 in the two-phase decoder):
    // every block counts its own valid pixels, the finalize kernel merges partials of unequal counts (never folded)
    const bool no_ragged_tiles = kn.gn_no_ragged_tiles;
    const bool raggedN = !no_fold && !no_ragged && !no_ragged_tiles && !c.up2 && !ragged1 && H * W > GN_TILE_PIXELS;
    const bool prod_ok = variant == CV_F64 || variant == CV_F32 || variant == CV_B64 ||
                         (variant == CV_B1 && !no_fold && c.ct_per_block == 0 && !c.w2 &&
                          ((H * W) % GN_TILE_PIXELS == 0 || ragged1 || raggedN));
    if (!((!premul || ragged1 || raggedN) && prod_ok && ((long)H * W >= min_hw || ragged1))) return false;
    const int BW = 1 << c.bw_log2, BH = GN_TILE_PIXELS / BW;
    // (phase form of an upsampling conv: tiles are SOURCE tiles, each computed for four output phases)
    const int um = c.up2 ? 2 : 1;
    const int tiles = c.tiles_x * c.tiles_y * (c.up2 ? 4 : 1);
    // the 128-pixel tiles cover the plane exactly (1x1: tiles of 128 consecutive pixels)
    const bool exact = c.ks == 1 ? (c.tiles_x * GN_TILE_PIXELS == H * W && c.tiles_y == 1)
                                 : (c.tiles_x * BW * um == W && c.tiles_y * BH * um == H);
    if (!(exact || ragged1 || raggedN) || (size_t)B * tiles * c.Cout * 8 > stat_cap) return false;
    // foldable into the consumer's prologue: few tiles, one group or power-of-two groups within a wave
    const int cg = c.Cout / groups;
    const int fold_tiles = (int)kn.gn_fold_tiles;
    // (a per-sample channel multiplier is applied by stage_ss_from_partials in its one-group branch only:
    //  with several groups the finalize kernel, which handles premul for any grouping, runs instead)
    r.foldable = !no_fold && (exact || ragged1) && tiles <= fold_tiles && c.Cout <= 512 && (!premul || groups == 1) &&
                 (groups == 1 || (cg <= 64 && (cg & (cg - 1)) == 0));
    r.tiles = tiles;
    r.mode = ragged1 ? GN_TILES_RAGGED1 : (exact ? GN_TILES_EXACT : GN_TILES_RAGGEDN);
    r.stat_count = ragged1 ? H * W : (exact ? 0 : -1);
    r.gn_count = ragged1 ? H * W : (exact ? GN_TILE_PIXELS : -1);
    r.geom = GnTileGeom{0, 0, 0, 0, 0};
    if (r.mode == GN_TILES_RAGGEDN) r.geom = GnTileGeom{c.tiles_x, c.bw_log2, H, W, c.ks == 1 ? 1 : 0};
    return true;
}

// ---------------------------------------------------------------------------
// FABlock2D with in_proj inside the sandwich (fa_fused.inc): the scales of the in_proj weight image and the plane groups a
// block walks.  One rule each for Planner::lower_fa and the op-level entry point lns_op_fa_fused.
// ---------------------------------------------------------------------------
struct FaWeightScale {
    float wscale;          // power of two the weights are multiplied by before their fp16 split (largest entry below 16000)
    float wrow_max;        // largest absolute row sum of W times (1 + 1e-6): the device multiplies it by max |G| in fp32, and
                           // the product must stay a bound of |P|
};
// wm: [planes][C] fp32.  An all-zero or non-finite matrix packs at scale 16000 / 1 and a row bound of at least 1.
static FaWeightScale fa_fused_weight_scale(const float* wm, int planes, int C) {
    float wmax = 0.0f, rowmax = 0.0f;
    for (int r = 0; r < planes; ++r) {
        float rs = 0.0f;
        for (int k = 0; k < C; ++k) { const float v = fabsf(wm[(size_t)r * C + k]); wmax = std::max(wmax, v); rs += v; }
        rowmax = std::max(rowmax, rs);
    }
    if (!(wmax > 0.0f) || !std::isfinite(rowmax)) { wmax = 1.0f; rowmax = std::max(rowmax, 1.0f); }
    return FaWeightScale{conv_f16_weight_scale(wmax), rowmax * (1.0f + 1e-6f)};
}
// Plane groups (of 16) per block, scheduling only.  requested > 0: that many, lowered to the next divisor of `groups`;
// 0 = automatic: all four groups of a head while the grid keeps two blocks per CU's worth of work.
static int fa_fused_gpb_rule(int requested, int groups, int B, int heads) {
    int gpb = requested > 0 ? std::min(requested, groups) : 4;
    while (gpb > 1 && (groups % gpb || (requested <= 0 && (long)B * heads * (groups / gpb) < 512))) --gpb;
    return gpb;
}

// ---------------------------------------------------------------------------
// Host pieces of the FABlock axis kernels and of ln_pe, shared by the planner and the op-level entry points
// (lns_op_fa_reducer, lns_op_fa_lrk, lns_op_ln_pe).
// ---------------------------------------------------------------------------
// src [rows][cols] -> dst [cols][rows]: the in-major layout of the reducer matrices (VX_TRANSPOSE2D) and of the positional
// table (VX_PE_T)
static void transpose_rows(float* dst, const float* src, size_t rows, size_t cols) {
    for (size_t r = 0; r < rows; ++r)
        for (size_t c = 0; c < cols; ++c) dst[c * rows + r] = src[r * cols + c];
}
// rotary table for LowRankKernel: pos = torch.linspace(0,1,n) (fp32 arithmetic of
// torch.linspace), t = pos * (scale/min_freq) = pos*64, freqs = t * inv_freq  (embedding.py:171-176)
// out: [half][n][2] (cos, sin), frequency-major
static void rotary_table_fill(int n, const float* inv_freq, int half, float* cs) {
    const float step = n > 1 ? (1.0f - 0.0f) / (float)(n - 1) : 0.0f;
    for (int i = 0; i < n; ++i) {
        // torch.linspace evaluates end - step * k with ONE rounding (a fused multiply-add; torch 2.10's CPU kernel, bit for bit):
        // the separately rounded product is an ulp off at 6160 of the 80199 positions of n = 2 .. 400, n = 15 and 16 among
        // them.  n == 1: torch.linspace(0, 1, 1) is [0], the start.
        float pos = (i < n / 2 || n == 1) ? (0.0f + step * (float)i) : std::fmaf(-step, (float)(n - 1 - i), 1.0f);
        const float t = pos * 64.0f;
        for (int d = 0; d < half; ++d) {
            const float f = t * inv_freq[d];
            cs[((size_t)d * n + i) * 2] = (float)std::cos((double)f);            // [half][n][2]: a wave reads one frequency's
            cs[((size_t)d * n + i) * 2 + 1] = (float)std::sin((double)f);        // row, positions on consecutive lanes
        }
    }
}
// LayerNorm output: |(x - mean) rstd| <= sqrt(C - 1), so |h| <= sqrt(C) max|gamma| + max|beta| + max|pe|
static float ln_pe_bound(int C, float g_absmax, float b_absmax, float pe_absmax) {
    return sqrtf((float)C) * g_absmax + b_absmax + pe_absmax;
}
static std::string fa_axis_limits(int C, int Hid, int Out) {
    return fmt("C = %d, Hid = %d, Out = %d: the MFMA form (C and Hid multiples of 32, C <= 256) needs %zu bytes of LDS, the "
               "scalar form %zu, the limit is %d", C, Hid, Out, fa_reducer_mfma_lds_bytes(C, Hid, Out),
               fa_reducer_scalar_lds_bytes(C, Hid, Out), (int)FA_AXIS_LDS_LIMIT);
}

// ---------------------------------------------------------------------------
// arena allocator for plan temporaries (offsets into the caller's workspace)
// ---------------------------------------------------------------------------
struct Arena {
    std::vector<std::pair<size_t, size_t>> free_;   // (offset, size), sorted by offset
    std::map<size_t, size_t> live;
    size_t top = 0, high = 0, base = 0;
    size_t alloc(size_t bytes) {
        bytes = round_up_sz(std::max<size_t>(bytes, 256), 256);
        for (size_t i = 0; i < free_.size(); ++i)
            if (free_[i].second >= bytes) {
                const size_t off = free_[i].first;
                if (free_[i].second == bytes) free_.erase(free_.begin() + i);
                else { free_[i].first += bytes; free_[i].second -= bytes; }
                live[off] = bytes;
                return off;
            }
        const size_t off = top;
        top += bytes;
        high = std::max(high, top);
        live[off] = bytes;
        return off;
    }
    void release(size_t off) {
        auto it = live.find(off);
        if (it == live.end()) throw std::runtime_error("arena: double free");
        size_t sz = it->second;
        live.erase(it);
        auto pos = std::lower_bound(free_.begin(), free_.end(), std::make_pair(off, (size_t)0));
        pos = free_.insert(pos, {off, sz});
        size_t i = pos - free_.begin();
        if (i + 1 < free_.size() && free_[i].first + free_[i].second == free_[i + 1].first) {
            free_[i].second += free_[i + 1].second;
            free_.erase(free_.begin() + i + 1);
        }
        if (i > 0 && free_[i - 1].first + free_[i - 1].second == free_[i].first) {
            free_[i - 1].second += free_[i].second;
            free_.erase(free_.begin() + i);
            --i;
        }
        if (free_[i].first + free_[i].second == top) { top = free_[i].first; free_.erase(free_.begin() + i); }
    }
};

// ---------------------------------------------------------------------------
// planner
// ---------------------------------------------------------------------------
struct TRef {
    uint64_t ptr = 0;      // tagged
    long bs = 0;           // batch stride (floats); <0: ext slot sentinel
    int C = 0, H = 0, W = 0;
    bool owned = false;    // arena allocation
    size_t ws_off = 0;
    // pending (un-materialised) transforms consumed by the next conv
    uint64_t ss = 0; size_t ss_off = 0; bool ss_owned = false;
    int act = ACT_NONE;
    int vH = 0, vW = 0; float sch = 0, scw = 0;   // virtual nearest resize
    int gn_lazy = -1;      // GroupNorm whose finalize op has not been emitted yet (index into Planner::lazy_ops): the consumer
                           // convolution merges the producer's tile partials itself, or flush_gn() emits the op
    // bound on |raw values| for the split-operand consumers: per-sample running maximum recorded by the producer
    // (tagged pointer to [B] unsigned) or an analytic constant (LayerNorm / InstanceNorm outputs); neither: unknown
    uint64_t amax = 0; float amax_const = 0.0f;
    // pending GroupNorm: |gamma| sqrt(n_group) + |beta| bounds the normalised tensor whatever the data (layer constant)
    float gn_bound = 0.0f;
    bool bounded() const { return amax != 0 || amax_const > 0.0f || (ss != 0 && gn_bound > 0.0f); }
    bool pending() const { return ss != 0 || act != ACT_NONE || vH != 0; }
};

enum { CLS_CONV3 = 0, CLS_CONV1, CLS_GN, CLS_LNPE, CLS_ATTN, CLS_FAPOOL, CLS_FARED, CLS_FALRK, CLS_FASAND, CLS_COND,
       CLS_SPECTRAL, CLS_MISC, CLS_COUNT };
static const char* kClsName[CLS_COUNT] = {"conv3x3_mfma", "conv1x1_mfma", "gn_stats", "ln_pe", "attention",
                                          "fa_pool", "fa_reducer", "fa_lrk", "fa_sandwich", "cond_embed",
                                          "spectral", "misc"};

// emit_conv: the geometry picked a kernel without the GELU prologue (input without a bound, patch too large for the
// f16x2 tile, a tuning knob): the planner falls back to a materialised activation (emit_apply)
struct NoGeluPrologue : std::runtime_error { using std::runtime_error::runtime_error; };

struct Planner {
    lns_engine* e;
    Plan* plan;
    int B;
    Arena arena;
    Planner(lns_engine* e_, Plan* p, int B_) : e(e_), plan(p), B(B_) {}

    // Scratch for GroupNorm partials written by convolution epilogues: allocated before any op so that it never
    // aliases a tensor (the producing conv writes it while its own inputs are still being read).
    // A RING of four regions: with the finalize step folded into the consumer convolution (below) the partials of a
    // tensor must survive until that consumer has run, while the consumer's own epilogue may already write the next
    // tensor's partials -- never into the region its blocks are still reading.  A region is reused four producers later;
    // if the GroupNorm it held has still not been consumed by then, the planner refuses (never a silent overwrite).
    static constexpr int STAT_RING = 4;
    uint64_t stat_ring[STAT_RING] = {0, 0, 0, 0};
    int stat_holder[STAT_RING] = {-1, -1, -1, -1};     // lazy GroupNorm (index) whose partials live in the region, or -1
    int stat_next = 0;
    uint64_t stat_scratch = 0;
    size_t stat_cap = 0;
    void init_stat_scratch() {
        if (knobs().gn_no_fuse) return;
        stat_cap = (size_t)B * 128 * e->cfg.Ly * e->cfg.Lx / GN_TILE_PIXELS * 8;   // C * H * W <= 128 * Ly * Lx
        // (a propagator-only engine has no field size: room for what the latent chain folds, <= 4 tiles x 512 channels,
        //  so that it takes the same per-layer decisions -- the same bits -- as the propagator inside a full model)
        stat_cap = std::max(stat_cap, (size_t)B * 4 * 512 * 8);
        for (int i = 0; i < STAT_RING; ++i) stat_ring[i] = tag(SP_WS, arena.alloc(stat_cap));
        stat_scratch = stat_ring[0];
    }
    uint64_t take_stat_region(const std::string& name, int lazy_index) {
        const int r = stat_next;
        stat_next = (stat_next + 1) % STAT_RING;
        if (stat_holder[r] >= 0 && !lazy_done[stat_holder[r]] && !lazy_folded[stat_holder[r]])
            throw std::runtime_error("GroupNorm partials ring exhausted at " + name);
        stat_holder[r] = lazy_index;
        return stat_ring[r];
    }

    // amax slots: one [B] unsigned vector per produced tensor, all in one region taken before any op (never aliased)
    enum { AMAX_SLOTS = 256 };
    size_t amax_off = 0; int amax_used = 0;
    void init_amax_region() {
        amax_off = arena.alloc((size_t)AMAX_SLOTS * B * LNS_AMAX_SUB * 4);
        plan->amax_off = amax_off;
    }
    uint64_t new_amax(const std::string& name) {
        if (amax_used >= AMAX_SLOTS) throw std::runtime_error("amax slots exhausted at " + name);
        plan->amax_names.push_back(name);
        return tag(SP_WS, amax_off + (size_t)(amax_used++) * B * LNS_AMAX_SUB * 4);
    }
    float vec_absmax(int id) const {
        if (id < 0) return 0.0f;
        float m = 0.0f;
        for (float v : e->params[e->pindex.at(e->vecs[id].key)].host) m = std::max(m, fabsf(v));
        return m;
    }

    uint64_t wt(size_t float_off) const { return tag(SP_WT, float_off * 4); }
    uint64_t vecp(int id) const { return id < 0 ? 0 : wt(e->vecs[id].off); }
    int vec_id(const std::string& key) const {
        for (size_t i = 0; i < e->vecs.size(); ++i) if (e->vecs[i].key == key) return (int)i;
        throw std::runtime_error("no vec pack for " + key);
    }
    TRef alloc_t(int C, int H, int W) {
        TRef t;
        t.C = C; t.H = H; t.W = W; t.bs = (long)C * H * W; t.owned = true;
        t.ws_off = arena.alloc((size_t)B * C * H * W * 4);
        t.ptr = tag(SP_WS, t.ws_off);
        return t;
    }
    void free_t(TRef& t) {
        if (t.owned) { arena.release(t.ws_off); t.owned = false; }
        if (t.ss_owned) { arena.release(t.ss_off); t.ss_owned = false; t.ss = 0; }
    }
    uint64_t const_ints(const std::vector<int>& v) {
        const size_t off = plan->consts_i.size();
        plan->consts_i.insert(plan->consts_i.end(), v.begin(), v.end());
        while (plan->consts_i.size() % 4) plan->consts_i.push_back(-1);
        return tag(SP_CT, off * 4) | (1ull << 55);   // bit 55: int segment (resolved in finish())
    }
    uint64_t const_floats(const std::vector<float>& v) {
        const size_t off = plan->consts_f.size();
        plan->consts_f.insert(plan->consts_f.end(), v.begin(), v.end());
        while (plan->consts_f.size() % 4) plan->consts_f.push_back(0.f);
        return tag(SP_CT, off * 4) | (1ull << 54);   // bit 54: float segment
    }
    void trace(const std::string& name, const TRef& t) {
        Op op;
        op.type = OP_TRACE; op.name = name; op.cls = CLS_MISC;
        op.t_ptr = t.ptr; op.t_bs = t.bs; op.tC = t.C; op.tH = t.H; op.tW = t.W;
        plan->ops.push_back(op);
    }

    // GroupNorm fed by a convolution's tile partials: the finalize op is held back (lazy) so that a split-operand
    // consumer can fold it into its prologue (ConvArgs::gn_part); anything else that reads the table flushes it first
    std::vector<Op> lazy_ops;
    std::vector<char> lazy_done, lazy_folded;
    void flush_gn(const TRef& x) {
        if (x.gn_lazy >= 0 && !lazy_done[x.gn_lazy]) { plan->ops.push_back(lazy_ops[x.gn_lazy]); lazy_done[x.gn_lazy] = 1; }
    }

    // GroupNorm statistics of a materialised tensor -> pending (scale, shift) on it
    void emit_gn(TRef& x, int groups, float eps, int vg, int vb, uint64_t premul, const std::string& name) {
        if (x.pending()) throw std::runtime_error("GroupNorm input must be materialised: " + name);
        if (x.C % groups) throw std::runtime_error("channels not divisible by groups: " + name);
        Op op;
        op.type = OP_GNSTATS; op.name = name; op.cls = CLS_GN;
        memset(&op.gn, 0, sizeof op.gn);
        op.gn.x = as_ptr<const float>(x.ptr); op.gn.x_bs = x.bs; op.gn.C = x.C; op.gn.HW = x.H * x.W;
        op.gn.groups = groups; op.gn.eps = eps;
        op.gn.gamma = as_ptr<const float>(vecp(vg)); op.gn.beta = as_ptr<const float>(vecp(vb));
        op.gn.premul = as_ptr<const float>(premul);
        // [B][C][2] scale/shift followed by [B][C][2] scratch of the two-stage path
        x.ss_off = arena.alloc((size_t)B * x.C * 4 * 4);
        x.ss = tag(SP_WS, x.ss_off); x.ss_owned = true;
        op.gn.ss = as_ptr<float>(x.ss); op.gn.B = B;
        op.bytes = 2.0 * B * x.C * x.H * x.W * 4;
        x.gn_bound = gn_output_bound(vg >= 0 ? vec_absmax(vg) : 1.0f, vb >= 0 ? vec_absmax(vb) : 0.0f, x.C / groups, x.H, x.W);
        // Fed by the 3x3 split-operand kernel right before it (nothing in between but traces), 128-pixel tiles
        // covering the plane exactly: the conv epilogue leaves per-tile (mean, M2) and this op only merges them.
        // Layer-static decision (gn_tile_rule), so results do not depend on the batch.
        Op* prod = nullptr;
        for (size_t i = plan->ops.size(); i-- > 0;) {
            // (traces and the conditional blocks' per-sample vector ops touch no activation tensor)
            const int ty = plan->ops[i].type;
            if (ty == OP_TRACE || ty == OP_CONDBLK || ty == OP_CONDBASE || ty == OP_VECLIN) continue;
            prod = &plan->ops[i];
            break;
        }
        GnTileRule r;
        if (stat_scratch && prod && prod->type == OP_CONV && prod->conv.y == as_ptr<float>(x.ptr) && prod->conv.Cout == x.C &&
            gn_tile_rule(r, prod->conv, prod->variant, x.H, x.W, groups, premul != 0, B, stat_cap)) {
            const int li = (int)lazy_ops.size();
            lazy_done.push_back(0); lazy_folded.push_back(0);
            const uint64_t region = take_stat_region(name, li);
            prod->conv.stat_part = as_ptr<float>(region);
            op.gn_tile_part = as_ptr<const float>(region);
            op.gn_tiles = r.tiles;
            op.gn_count = r.gn_count;
            if (r.mode == GN_TILES_RAGGEDN) op.gn_geom = r.geom;
            if (r.mode != GN_TILES_EXACT) prod->conv.stat_count = r.stat_count;
            // a batch-chunked producer: every chunk's launch leaves the partials of its own samples
            if (prod->chunk_group > 0)
                for (Op& o : plan->ops)
                    if (o.type == OP_CONV && o.chunk_group == prod->chunk_group) {
                        o.conv.stat_part = prod->conv.stat_part; o.conv.stat_count = prod->conv.stat_count;
                    }
            op.bytes = 2.0 * B * r.tiles * x.C * 8;
            lazy_ops.push_back(op);
            if (r.foldable) { x.gn_lazy = li; return; }
            lazy_done[li] = 1;                       // finalize right away (below)
        }
        plan->ops.push_back(op);
    }

    // fused conv; consumes the pending transforms of `in`
    // fuse_pack >= 0: a following 1x1 conv (64 -> 64) applied in the epilogue of this one
    static bool can_fuse_1x1(const ConvPack& first, const ConvPack& second) {
        return !knobs().no_fuse_1x1 && first.cout == 64 && second.k == 1 && second.cin == 64 && second.cout == 64;
    }
    // (i) the kernel form of a conv launch, from the layer's facts and the process switches alone: the tiling, the form of the
    // upsampling conv (ConvArgs::up2: 0 none, 1 one block per output phase, 2 resident patch, 3 quad phase, 4 dual phase)
    // and the input-stationary 1x1's cout tiles per block.  Hv x Wv: the plane the convolution sees (the phase form: the
    // source).  Every switch read of a conv launch is here; throws before anything is allocated or emitted.
    struct ConvForm { ConvGeom g; int up2, ct_per_block, Hv, Wv; };
    static ConvForm conv_form(const ConvPack& pk, const TRef& in, int B, int k, int stride, int dil, const int* pad, int act_out,
                              bool has_res, bool has_badd, bool fused, bool up2_dual, const std::string& name) {
        const Knobs& kn = knobs();
        ConvForm f;
        f.Hv = in.vH ? in.vH : in.H; f.Wv = in.vW ? in.vW : in.W;
        // 3x3 over an exactly 2x nearest-upsampled tensor: the phase-decomposed four-tap form (conv3_bf16x3_kernel, NTAP = 4)
        // -- tiles, patch and maps are those of a plain pad-1 3x3 convolution of the SOURCE; a per-layer rule
        // (LNS_CONV_FP32_MFMA, strict-fp32 runs: no split-operand kernels)
        const bool up2 = k == 3 && stride == 1 && dil == 1 && in.vH == 2 * in.H && in.vW == 2 * in.W && pk.has_wu && pk.f16 &&
                         pad[0] == 1 && pad[1] == 1 && pad[2] == 1 && pad[3] == 1 && in.bounded() && pk.cout > 32 && !kn.conv_fp32_mfma;
        if (up2) { f.Hv = in.H; f.Wv = in.W; }
        ConvGeom& g = f.g;
        const bool thin_ok = !has_res && !has_badd && act_out == ACT_NONE && !fused && !in.vH &&
                             (in.act == ACT_NONE || (in.act == ACT_SWISH && in.ss != 0));
        // split-operand kernels only where the input carries a bound for the dynamic activation scale (tensors
        // handed in by the caller do not: those few convolutions stay on the fp32 matrix instruction)
        auto tiling = [&](ConvGeom& gg, int force_variant, int force_bw_log2 = -1) {
            return conv_geometry(gg, B, pk.cout, f.Hv, f.Wv, k, stride, dil, pad, pk.kc_log2, pk.Cout_pad, force_variant, fused,
                                 pk.has_wb && in.bounded(), pk.cin, pk.f16, thin_ok, force_bw_log2);
        };
        if (!tiling(g, -1)) throw std::runtime_error("no conv tiling for " + name);
        if (up2 && g.variant == CV_F32 && !tiling(g, CV_F64))      // (a small launch: the phase form exists for 64-cout tiles only)
            throw std::runtime_error("no conv tiling for " + name);
        if (up2 && g.variant != CV_F64) throw std::runtime_error("phase form needs the f16x2 64-cout tiles: " + name);
        // what the forms' predicates (convuq_fits, convur_fits, convud_fits) read of a launch
        ConvArgs probe;
        memset(&probe, 0, sizeof probe);
        probe.ks = 3; probe.stride = 1; probe.dil = 1; probe.up2 = 1; probe.wb = &probe; probe.Cin_pad = pk.Cin_pad;
        probe.Cout = pk.cout; probe.Hout = 2 * in.H; probe.Wout = 2 * in.W;
        if (has_res) probe.res = reinterpret_cast<const float*>(&probe);
        // Round 4: the quad-phase form of the upsampling conv (conv3_up2q.inc: the patch staged once, four phases per block,
        // two blocks per CU) wants 8 x 16 source tiles -- a 10 x 18 patch of 8 stages is what fits beside its weight ring in
        // 80 KB.  MEASURED (profiles/r04_up2q_time.txt): the plain 64 -> 64 layer at 128^2 213.5 -> 197.6 us, but the layer the
        // decoder runs -- the same conv with the fused 1x1 -- 271 -> 278 us (its epilogue spills 96 registers at two waves per
        // SIMD) and the 64-channel UpSampleBlock conv 48.5 -> 49.0 us: rollout 34.6k -> 34.3k.  Opt-in (LNS_UP2_QUAD=1) in
        // -DLNS_EXPERIMENTAL builds only; a per-layer rule (Cin_pad in {16, 32, 48, 64}, no residual, the tiling exists).
        bool quad = false;
        ConvGeom gq;
        if (up2 && kn.up2_quad && !has_res && pk.Cin_pad <= 64 && pk.Cin_pad % 16 == 0 && tiling(gq, CV_F64, 4)) {
            probe.PH = gq.PH; probe.PW = gq.PW;
            if (convuq_fits(probe)) { g = gq; quad = true; }
        }
        if (in.act == ACT_GELU && ((g.variant != CV_F64 && g.variant != CV_F32) || up2 || fused))
            throw NoGeluPrologue("GELU prologue is only built into the f16x2 3x3 kernel: " + name);
        f.up2 = 0;
        if (up2) {
            g.Hout = 2 * in.H; g.Wout = 2 * in.W;
            probe.PH = g.PH; probe.PW = g.PW;
            f.up2 = 1;
            // narrow inputs: the split patch of ALL channels can stay in LDS while one block walks the four phases (same
            // bits, conv3_up2r.inc).  Measured SLOWER (fused 128^2 layer 294 - 299 vs 215 us, rollout 31.9k vs 33.4k): at
            // 147 KB of LDS a CU holds one block, and nothing overlaps its prologue, four epilogues and weight copies.
            // Kept as an opt-in variant (LNS_UP2_RESIDENT=1) with its parity tests.
            if (kn.up2_resident && convur_fits(probe)) f.up2 = 2;
            if (quad) f.up2 = 3;
            // the dual-phase form (conv3_up2d.inc: one block per source tile and row phase computes both column phases --
            // the patch staged once for the two, 8-byte stores of pixel pairs; same bits): a per-layer rule, "up2_dual"
            // (no fused 1x1)
            if (f.up2 == 1 && !fused && up2_dual && convud_fits(probe)) f.up2 = 4;
        }
        f.ct_per_block = 0;
        if (g.variant == CV_B1 && pk.Cin_pad <= 64 && g.cout_tiles >= 2 && !fused && !kn.conv1_no_stationary) {
            // input-stationary form; the number of cout tiles per block only changes the launch shape, never a bit:
            // as many cout tiles per block as still leave this many blocks (three fit a CU): LNS_CONV1S_MIN_BLOCKS
            int cpb = g.cout_tiles;
            while (cpb > 2 && (long)B * g.tiles_x * ((g.cout_tiles + cpb - 1) / cpb) < kn.conv1s_min_blocks) cpb = (cpb + 1) / 2;
            f.ct_per_block = cpb;
        }
        return f;
    }
    // (iii) what the launch costs and what it is called: nominal FLOP, bytes, executed matrix-pipe FLOP (every block runs whole
    // tiles, whole channel stages and whole tap slots), the form label of timing()
    static void conv_account(Op& op, const ConvForm& f, const ConvPack& pk, const TRef& in, int B, int k, bool has_res, bool fused) {
        const ConvGeom& g = f.g;
        const ConvVariantInfo vi = conv_variant_info(g.variant);
        const bool up2 = f.up2 != 0;
        op.flops = 2.0 * B * g.Hout * g.Wout * (double)pk.cout * pk.cin * k * k + (fused ? 2.0 * B * g.Hout * g.Wout * 64.0 * 64.0 : 0.0);
        op.bytes = 4.0 * B * ((double)in.C * in.H * in.W + (double)pk.cout * g.Hout * g.Wout * (has_res ? 2 : 1));
        const double tiles = (double)B * g.tiles_x * g.tiles_y * g.cout_tiles * vi.TM * vi.TN;
        if (cv_is_f16x2_3x3(g.variant)) {           // 3 products; 10 tap slots for 9 taps, or 4 phases x 4 taps
            op.mfma_flops = tiles * pk.Cin_pad * (up2 ? 4.0 * 4.0 : 10.0) * 3.0 * 2.0;
            op.form = up2 ? (fused ? "f16x2 3x3 four-tap phase form + fused 1x1" : "f16x2 3x3 four-tap phase form")
                          : (fused ? "f16x2 3x3 nine-tap + fused 1x1" : "f16x2 3x3 nine-tap");
            if (fused) op.mfma_flops += tiles * (up2 ? 4.0 : 1.0) * 64.0 * 3.0 * 2.0;
        } else if (g.variant == CV_B64 || g.variant == CV_B32) {
            op.mfma_flops = tiles * pk.Cin_pad * 10.0 * 6.0 * 2.0; op.form = "bf16x3 3x3 nine-tap";
        } else if (g.variant == CV_B1) {
            const int cp32 = (pk.Cin_pad + 31) / 32 * 32;
            op.mfma_flops = tiles * cp32 * (convb1_is_f16() ? 3.0 : 6.0) * 2.0;
            op.form = f.ct_per_block ? "f16x2 1x1 input-stationary" : (fused ? "f16x2 1x1 + fused 1x1" : "f16x2 1x1 streaming");
            if (fused) op.mfma_flops += tiles * 64.0 * 3.0 * 2.0;
        } else if (g.variant == CV_THIN) {
            op.form = "thin 1x1 projection (VALU)";
        } else {
            op.mfma_flops = tiles * pk.Cin_pad * (double)(k * k) * 2.0 + (fused ? tiles * 64.0 * 2.0 : 0.0);
            op.form = k == 3 ? "fp32 MFMA 3x3" : "fp32 MFMA 1x1";
        }
    }
    TRef emit_conv(const TRef& in, int pack_id, int k, int stride, int dil, const int* pad, int my, int mx,
                   int act_out, const TRef* res, uint64_t badd, const TRef* out_forced, const std::string& name,
                   int fuse_pack = -1, bool want_amax = true) {
        const ConvPack& pk = e->packs[pack_id];
        if (pk.cin != in.C) throw std::runtime_error(fmt("%s: input has %d channels, conv expects %d", name.c_str(), in.C, pk.cin));
        // (i) -- thrown before anything is allocated or emitted: a caller may catch NoGeluPrologue and materialise the activation
        const ConvForm f = conv_form(pk, in, B, k, stride, dil, pad, act_out, res != nullptr, badd != 0, fuse_pack >= 0,
                                     e->opt_up2_dual != 0, name);
        const ConvGeom& g = f.g;
        const bool up2 = f.up2 != 0;
        // (ii) the launch arguments
        std::vector<int> rm, cm;
        if (k == 3) conv_tile_maps(rm, cm, g, stride, in.H, in.W, f.Hv, f.Wv, up2 ? 0.0f : in.sch, up2 ? 0.0f : in.scw, pad, my, mx);
        else if (in.vH) throw std::runtime_error("1x1 conv of a resized tensor is not supported: " + name);
        TRef out;
        if (out_forced) out = *out_forced;
        else out = alloc_t(pk.cout, g.Hout, g.Wout);
        if (out.C != pk.cout || out.H != g.Hout || out.W != g.Wout)
            throw std::runtime_error(fmt("%s: output shape mismatch (%d,%d,%d) vs (%d,%d,%d)", name.c_str(), out.C, out.H,
                                         out.W, pk.cout, g.Hout, g.Wout));
        if (res && (res->C != out.C || res->H != out.H || res->W != out.W || res->pending()))
            throw std::runtime_error("residual shape mismatch: " + name);
        Op op;
        op.type = OP_CONV; op.name = name; op.cls = k == 3 ? CLS_CONV3 : CLS_CONV1; op.variant = g.variant;
        ConvArgs& a = op.conv;
        memset(&a, 0, sizeof a);
        conv_set_geometry(a, g, B, in.C, in.H, in.W, pk.cout, k, stride, dil, pk.Cin_pad, pk.Cout_pad);
        a.x = as_ptr<const float>(in.ptr); a.x_bs = in.bs;        // (strides of the TRefs: an external slot's is a sentinel)
        a.y = as_ptr<float>(out.ptr); a.y_bs = out.bs;
        a.w = as_ptr<const float>(wt(pk.w_off));
        if (g.variant >= CV_B64) a.wb = as_ptr<const void>(wt(up2 ? pk.wu_off : pk.wb_off));   // CV_B32 included
        a.up2 = f.up2;
        a.ct_per_block = f.ct_per_block;
        a.bias = pk.has_bias ? as_ptr<const float>(wt(pk.b_off)) : nullptr;
        a.ss = as_ptr<const float>(in.ss);
        if (in.gn_lazy >= 0 && !lazy_done[in.gn_lazy]) {
            // GroupNorm whose finalize step is still pending: the split-operand kernels merge the producer's tile partials in
            // their own prologue (no launch); every other consumer gets the finalize op now
            if (g.variant == CV_F64 || g.variant == CV_F32 || g.variant == CV_B1) {
                const Op& lo = lazy_ops[in.gn_lazy];
                conv_fold_gn(a, lo.gn_tile_part, lo.gn_tiles, lo.gn_count, lo.gn.groups, lo.gn.eps, lo.gn.premul, lo.gn.gamma, lo.gn.beta);
                lazy_folded[in.gn_lazy] = 1;
            } else {
                flush_gn(in);
            }
        }
        a.act_in = in.act; a.act_out = act_out;
        if (k == 3) {
            a.rowmap = as_ptr<const int>(const_ints(rm));
            a.colmap = as_ptr<const int>(const_ints(cm));
            conv_set_map_arith(a, g.variant, k, in.H, in.W, f.Hv, f.Wv, pad, my, mx);
        }
        if (res) { a.res = as_ptr<const float>(res->ptr); a.res_bs = res->bs; }
        a.badd = as_ptr<const float>(badd);
        a.unscale = conv_unscale(g.variant, up2 ? pk.wscale_up : pk.wscale);   // x 1/S in the kernel
        if (in.ss != 0 && in.gn_bound > 0.0f) conv_set_final_bound(a, in.gn_bound);   // GroupNorm output: layer constant
        else {
            a.amax_in = as_ptr<const unsigned>(in.amax); a.amax_in_const = in.amax_const;
            if (!in.amax && in.ss == 0) a.bound_final = 1;     // analytic bound of a raw tensor (LayerNorm / InstanceNorm output)
        }
        out.amax = 0; out.amax_const = 0.0f; out.gn_bound = 0.0f;
        // a tensor written to a caller's buffer (the plan's output) is always recorded: nobody scales by it, but
        // lns_check_finite must see a NaN born in the last layer as well
        if ((want_amax && g.variant != CV_THIN) || out_forced) { out.amax = new_amax(name); a.amax_out = as_ptr<unsigned>(out.amax); }
        if (fuse_pack >= 0) {
            const ConvPack& p2 = e->packs[fuse_pack];
            if (!can_fuse_1x1(pk, p2)) throw std::runtime_error("cannot fuse 1x1 into " + name);
            a.w2 = as_ptr<const float>(wt(p2.w_off));
            a.bias2 = p2.has_bias ? as_ptr<const float>(wt(p2.b_off)) : nullptr;
            a.Cout2_pad = p2.Cout_pad;
            {   // scale of the fused 1x1 weights for the fp16 split in the epilogue (max |w2| just below 2^14)
                float mx = 0.0f;
                for (const std::string& key : p2.wkeys)
                    for (float v : e->params[e->pindex.at(key)].host) mx = std::max(mx, fabsf(v));
                a.w2scale = (mx > 0.0f && std::isfinite(mx)) ? conv_f16_weight_scale(mx) : 1.0f;
            }
        }
        conv_account(op, f, pk, in, B, k, res != nullptr, fuse_pack >= 0);      // (iii)
        plan->ops.push_back(op);
        return out;
    }
    TRef conv_same1(const TRef& in, int pack, int act_out, const TRef* res, const TRef* out_forced,
                    const std::string& name, int fuse_pack = -1, bool want_amax = true) {
        const int pad[4] = {0, 0, 0, 0};
        return emit_conv(in, pack, 1, 1, 1, pad, 0, 0, act_out, res, 0, out_forced, name, fuse_pack, want_amax);
    }
    TRef conv_same3(const TRef& in, int pack, int dil, int my, int mx, int act_out, const TRef* res, uint64_t badd,
                    const std::string& name, bool want_amax = true) {
        const int pad[4] = {dil, dil, dil, dil};
        return emit_conv(in, pack, 3, 1, dil, pad, my, mx, act_out, res, badd, nullptr, name, -1, want_amax);
    }

    // ---- composite modules ----------------------------------------------------
    // `raw_out`: the block's output will be read un-normalised by a split-operand convolution (next layer is a conv /
    // an up-sampling conv / a block with a channel_up) and needs the amax side channel; tensors that only feed
    // GroupNorm-prologue convolutions (analytic bound) or residual adds do not.
    TRef lower_res(const Layer& l, TRef x, bool raw_out) {
        if (x.pending()) throw std::runtime_error("ResidualBlock input must be materialised: " + l.name);
        TRef skip = x;
        bool skip_owned = false;
        if (l.chup >= 0) { skip = conv_same1(x, l.chup, ACT_NONE, nullptr, nullptr, l.name + ".channel_up", -1, false); skip_owned = true; }
        TRef xin = x; xin.owned = false;
        emit_gn(xin, 32, 1e-6f, l.g1, l.b1, 0, l.name + ".gn1");
        xin.act = ACT_SWISH;
        TRef h1 = conv_same3(xin, l.conv1, 1, l.mode_y, l.mode_x, ACT_NONE, nullptr, 0, l.name + ".conv1", false);
        free_t(xin);   // releases the stats buffer only (xin does not own x)
        emit_gn(h1, 32, 1e-6f, l.g2, l.b2, 0, l.name + ".gn2");
        h1.act = ACT_SWISH;
        TRef out = conv_same3(h1, l.conv2, 1, l.mode_y, l.mode_x, ACT_NONE, &skip, 0, l.name + ".conv2", raw_out);
        free_t(h1);
        if (skip_owned) free_t(skip);
        return out;
    }

    TRef lower_sa(const Layer& l, TRef x, bool raw_out) {
        if (x.pending()) throw std::runtime_error("SABlock input must be materialised");
        const int n = x.H * x.W, inner = l.heads * l.dim_head;
        if (l.pe >= 0 && n > l.pe_len) throw std::runtime_error("SABlock: more tokens than positional table rows");
        TRef h = alloc_t(x.C, x.H, x.W);
        h.amax_const = ln_pe_bound(x.C, vec_absmax(l.ln_g), vec_absmax(l.ln_b), vec_absmax(l.pe));
        {
            Op op;
            op.type = OP_LNPE; op.name = l.name + ".ln_pe"; op.cls = CLS_LNPE;
            memset(&op.ln, 0, sizeof op.ln);
            op.ln.x = as_ptr<const float>(x.ptr); op.ln.x_bs = x.bs; op.ln.C = x.C; op.ln.n = n; op.ln.eps = 1e-5f;
            op.ln.gamma = as_ptr<const float>(vecp(l.ln_g)); op.ln.beta = as_ptr<const float>(vecp(l.ln_b));
            op.ln.pe_t = as_ptr<const float>(vecp(l.pe)); op.ln.pe_stride = l.pe_len;
            op.ln.h = as_ptr<float>(h.ptr); op.ln.B = B;
            op.bytes = 2.0 * B * x.C * n * 4;
            plan->ops.push_back(op);
        }
        TRef qkv = conv_same1(h, l.qkv, ACT_NONE, nullptr, nullptr, l.name + ".qkv");
        free_t(h);
        TRef o = alloc_t(inner, x.H, x.W);
        o.amax = qkv.amax;          // softmax rows are convex weights: |o| <= max |v| <= max |qkv| of the sample
        {
            Op op;
            op.type = OP_ATTN; op.name = l.name + ".attn"; op.cls = CLS_ATTN;
            op.at.qkv = as_ptr<const float>(qkv.ptr); op.at.B = B; op.at.heads = l.heads; op.at.D = l.dim_head;
            op.at.n = n; op.at.scale = (float)std::pow((double)l.dim_head, -0.5); op.at.o = as_ptr<float>(o.ptr);
            op.at.amax_in = qkv.amax ? as_ptr<const unsigned>(qkv.amax) : nullptr;
            op.flops = 4.0 * B * l.heads * (double)n * n * l.dim_head;
            {
                const bool f16 = attn_is_f16(op.at);
                const double np_ = (n + 31) / 32 * 32;
                op.mfma_flops = 4.0 * B * l.heads * np_ * np_ * l.dim_head * (f16 ? 3.0 : 1.0);
                op.form = f16 ? "f16x2 attention" : "fp32 MFMA attention";
            }
            op.bytes = 4.0 * B * 4.0 * inner * n;
            plan->ops.push_back(op);
        }
        free_t(qkv);
        TRef out = conv_same1(o, l.proj, ACT_NONE, &x, nullptr, l.name + ".proj_out", -1, raw_out);
        free_t(o);
        return out;
    }

    uint64_t rotary_table(int n, const std::string& invf_key) {
        const Param& p = e->params[e->pindex.at(invf_key)];
        const int half = (int)p.numel();
        std::vector<float> cs((size_t)n * half * 2);
        rotary_table_fill(n, p.host.data(), half, cs.data());
        return const_floats(cs);
    }

    // FABlock2D's three passes over the 512-plane tensor (in_proj writes it, the sandwich rewrites it in place, to_out reads
    // it: 537 MB at 64 x 64, B = 64 -- twice the Infinity Cache, so every pass goes to HBM) are re-issued per GROUP OF SAMPLES
    // small enough for the group's slice to stay in the cache from one kernel to the next: [in_proj, sandwich, to_out](chunk 0),
    // [...](chunk 1), ...  The ops in between (pooling, reducers, low-rank kernels) do not depend on in_proj and keep
    // their place; per-sample arithmetic is untouched (ConvArgs::b0), so the bits do not change.
    int next_chunk_group = 1;
    int fa_chunk_samples(size_t bytes_per_sample) const {          // 0: no chunking
        const long cap = (long)e->opt_fa_chunk_mb << 20;
        if (cap <= 0 || (long)bytes_per_sample * B <= cap) return 0;
        const int chunk = (int)std::max<long>(1, cap / (long)bytes_per_sample);
        return chunk >= B ? 0 : chunk;
    }
    void chunk_fa_chain(size_t inproj_at, size_t sandwich_at, size_t toout_at, size_t bytes_per_sample) {
        const int chunk = fa_chunk_samples(bytes_per_sample);
        if (!chunk) return;
        const Op a = plan->ops[inproj_at], s = plan->ops[sandwich_at], o = plan->ops[toout_at];
        if (a.type != OP_CONV || s.type != OP_FASAND || o.type != OP_CONV || !(inproj_at < sandwich_at && sandwich_at < toout_at))
            throw std::runtime_error("chunk_fa_chain: unexpected op order");
        plan->ops.erase(plan->ops.begin() + toout_at);
        plan->ops.erase(plan->ops.begin() + sandwich_at);
        plan->ops.erase(plan->ops.begin() + inproj_at);
        const int ga = next_chunk_group++, go = next_chunk_group++;
        for (int b0 = 0; b0 < B; b0 += chunk) {
            const int nb = std::min(chunk, B - b0);
            const double share = (double)nb / B;
            Op ca = a, cs = s, co = o;
            ca.conv.b0 = b0; ca.conv.B = nb; ca.chunk_group = ga;
            cs.fs.b0 = b0; cs.fs.B = nb;
            co.conv.b0 = b0; co.conv.B = nb; co.chunk_group = go;
            for (Op* c : {&ca, &cs, &co}) { c->flops *= share; c->bytes *= share; c->mfma_flops *= share; }
            plan->ops.push_back(ca); plan->ops.push_back(cs); plan->ops.push_back(co);
        }
    }

    TRef lower_fa(const Layer& l, TRef x, bool raw_out) {
        if (x.pending()) throw std::runtime_error("FABlock2D input must be materialised");
        const int C = x.C, H = x.H, W = x.W, heads = l.heads, dh = l.dim_head, lat = l.fa_lat, DK = l.fa_dk;
        TRef xin = x; xin.owned = false;
        emit_gn(xin, 1, 1e-5f, l.fa_g, l.fa_b, 0, l.name + ".in_norm");
        // in_proj records max |u| per sample: the sandwich's f16x2 form scales its planes by it
        // round 4: in_proj inside the sandwich kernel (fa_fused.inc) -- the plane tensor is only ever the sandwich's OUTPUT
        const Knobs& kn = knobs();
        const bool fused_off = kn.fa_sandwich_fp32 || kn.conv_fp32_mfma || kn.conv1_fp32_mfma || kn.fa_sandwich_bf16x3;
        const bool no_small = kn.fa_fused_no_small;      // A/B knob: only the 64 x 64 block
        const bool fused_in = e->opt_fa_fused && !fused_off && fa_fused_fits(H, W, C, dh) && !(no_small && H < 64) && !e->packs[l.inproj].has_bias &&
                              e->packs[l.inproj].cout == heads * dh && xin.ss != 0 && xin.gn_bound > 0.0f;
        TRef uphi;
        size_t inproj_at = 0, gs_off = 0;
        uint64_t amax_g = 0;
        if (fused_in) {
            flush_gn(xin);                  // the pre-pass reads the finished (scale, shift) table
            gs_off = arena.alloc(fa_fused_gs_bytes(B, H, W, C));
            amax_g = new_amax(l.name + ".in_split");
            Op op;
            op.type = OP_FAGSPLIT; op.name = l.name + ".in_split"; op.cls = CLS_FASAND;
            op.fg.x = as_ptr<const float>(xin.ptr); op.fg.x_bs = xin.bs; op.fg.Cin = C; op.fg.HW = H * W;
            op.fg.ss = as_ptr<const float>(xin.ss); op.fg.bound = xin.gn_bound;
            op.fg.gs = as_ptr<void>(tag(SP_WS, gs_off)); op.fg.amax_out = as_ptr<unsigned>(amax_g); op.fg.B = B;
            op.bytes = 8.0 * B * C * H * W;
            op.form = "FABlock input split (VALU)";
            plan->ops.push_back(op);
            uphi = alloc_t(heads * dh, H, W);
        } else {
            uphi = conv_same1(xin, l.inproj, ACT_NONE, nullptr, nullptr, l.name + ".in_proj", -1, true);
            inproj_at = plan->ops.size() - 1;
        }
        // axis pooling of the NORMALISED INPUT: to_in (1x1, no bias) and the reducers' first Linear commute with the mean over
        // an axis, so the pool reads xin through its (scale, shift) table and the reducers apply W_x W_toin / W_y W_toin
        // (VecPack::key2) -- the full-resolution to_in conv and its output tensor do not exist.  in_proj may have merged the
        // GroupNorm partials in its own prologue; the pool needs the finished table.
        flush_gn(xin);
        const size_t mx_off = arena.alloc((size_t)B * H * C * 4), my_off = arena.alloc((size_t)B * W * C * 4);
        {
            Op op;
            op.type = OP_FAPOOL; op.name = l.name + ".pool"; op.cls = CLS_FAPOOL;
            op.fp.x = as_ptr<const float>(xin.ptr); op.fp.x_bs = xin.bs; op.fp.ss = as_ptr<const float>(xin.ss);
            op.fp.B = B; op.fp.C = C; op.fp.H = H; op.fp.W = W;
            op.fp.mx = as_ptr<float>(tag(SP_WS, mx_off)); op.fp.my = as_ptr<float>(tag(SP_WS, my_off));
            op.bytes = 4.0 * B * C * H * W;
            plan->ops.push_back(op);
        }
        // (chunked: in_proj is re-issued AFTER the pooling / reducer / low-rank ops, so the GroupNorm table it reads must
        //  outlive their allocations)
        const bool fused_out = !kn.fa_no_fuse_to_out && can_fuse_1x1(e->packs[l.out1], e->packs[l.out3]);
        const bool will_chunk = !fused_in && fused_out && fa_chunk_samples((size_t)heads * dh * H * W * 4) > 0;
        if (!will_chunk) free_t(xin);
        // PoolingReducer of both axes in ONE launch, rotary + q k^T of both axes in one more
        // (LNS_FA_NO_MERGE restores one launch per axis)
        const bool merge = !kn.fa_no_merge && fa_reducer_fits(C, 2 * C, lat, true);
        // no form for this shape: say so here, by name, not at the first launch
        if (!merge && !fa_reducer_fits(C, 2 * C, lat, false))
            throw std::runtime_error(l.name + ": no PoolingReducer kernel for " + fa_axis_limits(C, 2 * C, lat));
        if (!fa_lrk_fits(DK, std::max(H, W)))
            throw std::runtime_error(l.name + fmt(": no LowRankKernel kernel for DK = %d, n = %d: q' and k' need %zu bytes of LDS, the limit is %d",
                                                  DK, std::max(H, W), fa_lrk_lds_bytes(DK, std::max(H, W)), (int)FA_AXIS_LDS_LIMIT));
        auto fill_reducer = [&](FaReducerArgs& fr, int ax) {
            const int* r = ax == 0 ? l.rx : l.ry;
            const int n = ax == 0 ? H : W;
            memset(&fr, 0, sizeof fr);
            fr.m = as_ptr<const float>(tag(SP_WS, ax == 0 ? mx_off : my_off));
            fr.rows = (long)B * n; fr.n = n; fr.C = C; fr.Hid = 2 * C; fr.Out = lat;
            fr.win_t = as_ptr<const float>(vecp(r[0])); fr.ln_g = as_ptr<const float>(vecp(r[1]));
            fr.ln_b = as_ptr<const float>(vecp(r[2])); fr.w1_t = as_ptr<const float>(vecp(r[3]));
            fr.w2_t = as_ptr<const float>(vecp(r[4])); fr.b2 = as_ptr<const float>(vecp(r[5]));
        };
        // (fusing to_qk into the reducer as a fourth chained GEMM was measured slower: 163 us per launch against
        //  2 x 25 us for the stand-alone convolutions, the projection has too little parallelism per 32-row block)
        TRef qkx, qky;
        {
            TRef ux = alloc_t(lat, 1, H), uy = alloc_t(lat, 1, W);
            ux.amax = new_amax(l.name + ".to_x"); uy.amax = new_amax(l.name + ".to_y");
            if (merge) {
                Op op;
                op.type = OP_FARED2; op.name = l.name + ".to_xy"; op.cls = CLS_FARED;
                fill_reducer(op.fr, 0); fill_reducer(op.fr2, 1);
                op.fr.u = as_ptr<float>(ux.ptr); op.fr2.u = as_ptr<float>(uy.ptr);
                op.fr.amax_out = as_ptr<unsigned>(ux.amax); op.fr2.amax_out = as_ptr<unsigned>(uy.amax);
                op.flops = 2.0 * B * (H + W) * ((double)C * C + 2.0 * C * C + 2.0 * C * lat);
                plan->ops.push_back(op);
            } else {
                for (int ax = 0; ax < 2; ++ax) {
                    Op op;
                    op.type = OP_FARED; op.name = l.name + (ax == 0 ? ".to_x" : ".to_y"); op.cls = CLS_FARED;
                    fill_reducer(op.fr, ax);
                    op.fr.u = as_ptr<float>((ax == 0 ? ux : uy).ptr);
                    op.fr.amax_out = as_ptr<unsigned>((ax == 0 ? ux : uy).amax);
                    op.flops = 2.0 * B * (ax == 0 ? H : W) * ((double)C * C + 2.0 * C * C + 2.0 * C * lat);
                    plan->ops.push_back(op);
                }
            }
            arena.release(mx_off); arena.release(my_off);
            qkx = conv_same1(ux, l.qkx, ACT_NONE, nullptr, nullptr, l.name + ".lrk_x.to_qk", -1, false);
            qky = conv_same1(uy, l.qky, ACT_NONE, nullptr, nullptr, l.name + ".lrk_y.to_qk", -1, false);
            free_t(ux); free_t(uy);
        }
        const size_t kx_off = arena.alloc((size_t)B * heads * H * H * 4), ky_off = arena.alloc((size_t)B * heads * W * W * 4);
        {
            Op op;
            op.type = merge ? OP_FALRK2 : OP_FALRK; op.cls = CLS_FALRK;
            for (int ax = 0; ax < 2; ++ax) {
                const int n = ax == 0 ? H : W;
                FaLrkArgs& fl = (merge && ax == 1) ? op.fl2 : op.fl;
                fl.qk = as_ptr<const float>((ax == 0 ? qkx : qky).ptr); fl.B = B; fl.heads = heads; fl.DK = DK;
                fl.n = n; fl.cs = as_ptr<const float>(rotary_table(n, ax == 0 ? l.invf_x : l.invf_y));
                fl.kmat = as_ptr<float>(tag(SP_WS, ax == 0 ? kx_off : ky_off));
                if (!merge) {
                    op.name = l.name + (ax == 0 ? ".lrk_x" : ".lrk_y");
                    op.flops = 2.0 * B * heads * (double)n * n * DK;
                    plan->ops.push_back(op);
                }
            }
            if (merge) {
                op.name = l.name + ".lrk_xy";
                op.flops = 2.0 * B * heads * ((double)H * H + (double)W * W) * DK;
                plan->ops.push_back(op);
            }
        }
        free_t(qkx); free_t(qky);
        if (fused_in) {
            const ConvPack& pk = e->packs[l.inproj];
            const int planes = heads * dh;
            std::vector<float> wm((size_t)planes * C);
            {   // [planes][C] from the (possibly concatenated) state_dict tensors
                size_t row = 0;
                for (const std::string& key : pk.wkeys) {
                    const Param& p = e->params[e->pindex.at(key)];
                    if (p.numel() % (size_t)C) throw std::runtime_error("in_proj weight shape: " + key);
                    std::copy(p.host.begin(), p.host.end(), wm.begin() + row * C);
                    row += p.numel() / C;
                }
                if ((int)row != planes) throw std::runtime_error("in_proj weight rows: " + l.name);
            }
            const FaWeightScale ws = fa_fused_weight_scale(wm.data(), planes, C);
            std::vector<float> img(fa_fused_weight_bytes(planes, C) / 4);
            fa_fused_pack_weight(img.data(), wm.data(), planes, C, ws.wscale);
            Op op;
            op.type = OP_FAFUSED; op.name = l.name + ".sandwich"; op.cls = CLS_FASAND;
            op.ff.gs = as_ptr<const void>(tag(SP_WS, gs_off)); op.ff.amax_g = as_ptr<const unsigned>(amax_g); op.ff.bound = xin.gn_bound;
            op.ff.wp = as_ptr<const void>(const_floats(img)); op.ff.w_inv = 1.0f / ws.wscale;
            op.ff.wrow_max = ws.wrow_max;
            op.ff.kx = as_ptr<const float>(tag(SP_WS, kx_off)); op.ff.ky = as_ptr<const float>(tag(SP_WS, ky_off));
            op.ff.B = B; op.ff.heads = heads; op.ff.C = dh; op.ff.Cin = C; op.ff.H = H; op.ff.W = W; op.ff.eps = 1e-5f; op.ff.instnorm = 1;
            op.ff.out = as_ptr<float>(uphi.ptr);
            op.ff.b_rev = kn.fa_no_reverse ? 0 : 1;
            op.ff.single_buffer = e->opt_fa_fused == 1 ? 1 : (e->opt_fa_fused == 3 ? 2 : 0);
            // plane groups per block (scheduling only; "fa_fused_gpb" / LNS_FA_FUSED_GPB)
            op.ff.gpb = fa_fused_gpb_rule(e->opt_fa_fused_gpb, dh / 16, B, heads);
            op.flops = 2.0 * B * heads * dh * ((double)H * W * W + (double)H * H * W) + 2.0 * B * planes * (double)C * H * W;
            op.bytes = 4.0 * B * ((double)planes + C) * H * W;
            op.mfma_flops = (2.0 * B * heads * dh * ((double)H * W * W + (double)H * H * W) + 2.0 * B * planes * (double)C * H * W) * 3.0;
            op.form = "f16x2 FABlock in_proj + sandwich";
            plan->ops.push_back(op);
            arena.release(gs_off);
        } else {
            Op op;
            op.type = OP_FASAND; op.name = l.name + ".sandwich"; op.cls = CLS_FASAND;
            op.fs.u = as_ptr<const float>(uphi.ptr); op.fs.kx = as_ptr<const float>(tag(SP_WS, kx_off));
            op.fs.ky = as_ptr<const float>(tag(SP_WS, ky_off)); op.fs.B = B; op.fs.heads = heads; op.fs.C = dh;
            op.fs.H = H; op.fs.W = W; op.fs.eps = 1e-5f; op.fs.instnorm = 1; op.fs.out = as_ptr<float>(uphi.ptr);
            op.fs.amax_u = uphi.amax ? as_ptr<const unsigned>(uphi.amax) : nullptr;
            op.fs.b_rev = kn.fa_no_reverse ? 0 : 1;
            op.flops = 2.0 * B * heads * dh * ((double)H * W * W + (double)H * H * W);
            op.bytes = 8.0 * B * heads * dh * H * W;
            {   // 32 x 32 tiles; the kernel is the launcher's choice (fa_sandwich_form): products per MFMA tile f16x2 3,
                // bf16x3 6 (fa_sandwich_b_kernel: hh, hm, mh, mm, hl, lh for U and again for Y), fp32 MFMA 1
                const double Hp = (H + 31) / 32 * 32, Wp = (W + 31) / 32 * 32;
                double products = 1.0;
                switch (fa_sandwich_form(op.fs)) {
                    case FA_SAND_F16X2: products = 3.0; op.form = "f16x2 FABlock sandwich"; break;
                    case FA_SAND_BF16X3: products = 6.0; op.form = "bf16x3 FABlock sandwich"; break;
                    case FA_SAND_BF16X3_3WAVE: products = 6.0; op.form = "bf16x3 FABlock sandwich (three waves)"; break;
                    case FA_SAND_FP32: op.form = "fp32 MFMA FABlock sandwich"; break;
                    default:      // no kernel for this shape: say so here, by name, not at the first launch
                        throw std::runtime_error(l.name + fmt(": no FABlock sandwich kernel for %d x %d planes (32 x 32 tiles: 1x1, 1x2, 2x1, 2x2, 2x3)", H, W));
                }
                op.mfma_flops = 2.0 * B * heads * dh * (Hp * Wp * Wp + Hp * Hp * Wp) * products;
            }
            plan->ops.push_back(op);
        }
        const size_t sandwich_at = plan->ops.size() - 1;
        // (chunked: the sandwich of chunk i + 1 runs after to_out of chunk i, so Kx / Ky must outlive to_out's allocations)
        if (!will_chunk) { arena.release(kx_off); arena.release(ky_off); }
        // InstanceNorm output (biased variance over H*W values): |y| <= sqrt(H*W - 1)
        uphi.amax = 0; uphi.amax_const = sqrtf((float)(H * W));
        TRef out;
        if (fused_out) {      // (LNS_FA_NO_FUSE_TO_OUT: tuning knob; measured: fused wins)
            // to_out.1 (512 -> 64, GELU) and to_out.3 (64 -> 64) + skip in ONE kernel
            out = conv_same1(uphi, l.out1, ACT_GELU, &x, nullptr, l.name + ".to_out.1+3", l.out3, raw_out);
            free_t(uphi);
            if (will_chunk) {
                chunk_fa_chain(inproj_at, sandwich_at, plan->ops.size() - 1, (size_t)heads * dh * H * W * 4);
                free_t(xin); arena.release(kx_off); arena.release(ky_off);
            }
        } else {
            TRef t1 = conv_same1(uphi, l.out1, ACT_GELU, nullptr, nullptr, l.name + ".to_out.1");
            free_t(uphi);
            out = conv_same1(t1, l.out3, ACT_NONE, &x, nullptr, l.name + ".to_out.3", -1, raw_out);
            free_t(t1);
        }
        return out;
    }

    // DilatedResidualBlock: train_stage2_ns2d.py:25-53
    TRef lower_propblock(const Layer& l, TRef x, bool raw_out) {
        TRef xin = x; xin.owned = false;
        emit_gn(xin, 1, 1e-5f, l.p_g1, l.p_b1, 0, l.name + ".conv.0");
        TRef h1 = conv_same3(xin, l.p_c1, 1, l.mode_y, l.mode_x, ACT_GELU, nullptr, 0, l.name + ".conv.1");
        free_t(xin);
        TRef h2 = conv_same3(h1, l.p_c3, l.dil, l.mode_y, l.mode_x, ACT_GELU, nullptr, 0, l.name + ".conv.3");
        free_t(h1);
        TRef x1 = conv_same3(h2, l.p_c5, 1, l.mode_y, l.mode_x, ACT_NONE, &x, 0, l.name + ".conv.5", false);
        free_t(h2);
        TRef xin2 = x1; xin2.owned = false;
        emit_gn(xin2, 1, 1e-5f, l.p_g2, l.p_b2, 0, l.name + ".ffn.0");
        TRef f1 = conv_same1(xin2, l.p_f1, ACT_GELU, nullptr, nullptr, l.name + ".ffn.1");
        free_t(xin2);
        TRef out = conv_same1(f1, l.p_f3, ACT_NONE, &x1, nullptr, l.name + ".ffn.3", -1, raw_out);
        free_t(f1); free_t(x1);
        return out;
    }

    // materialise a pending GroupNorm scale/shift (+ activation) -- used where the consumer's
    // prologue cannot express it (GELU prologue of the conditional block)
    TRef emit_apply(TRef& x, int act, const std::string& name) {
        flush_gn(x);
        TRef y = alloc_t(x.C, x.H, x.W);
        Op op;
        op.type = OP_APPLY; op.name = name; op.cls = CLS_MISC;
        op.ap.x = as_ptr<const float>(x.ptr); op.ap.x_bs = x.bs; op.ap.ss = as_ptr<const float>(x.ss);
        op.ap.act = act; op.ap.y = as_ptr<float>(y.ptr); op.ap.B = B; op.ap.C = x.C; op.ap.HW = x.H * x.W;
        y.amax = new_amax(name); op.ap.amax_out = as_ptr<unsigned>(y.amax);
        op.bytes = 8.0 * B * x.C * x.H * x.W;
        plan->ops.push_back(op);
        return y;
    }

    // conditional propagator, step-invariant part: cond_emb_proj(fourier_embedding(param))
    // train_stage2_twophase_conditional.py:116, modules/cond_utils.py:19-38
    uint64_t cond_ce = 0; size_t cond_ce_off = 0; bool cond_ce_live = false;
    // The embedding buffers (ce, and emb / mul of every block) depend on `param` only and are reused by the steps
    // after the first one of a rollout: they come out of a pool taken from the arena BEFORE any op is lowered, so no
    // tensor of the plan -- earlier or later -- can ever be placed on them.
    size_t cond_pool_off = 0, cond_pool_cap = 0, cond_pool_used = 0;
    void init_cond_pool() {
        const lns_config& c = e->cfg;
        if (c.cond_emb_dim <= 0 || c.prop_n_block <= 0) return;
        cond_pool_cap = round_up_sz((size_t)B * c.cond_emb_dim * 4, 256) +
                        (size_t)c.prop_n_block * 2 * round_up_sz((size_t)B * std::max(c.prop_n_embd, 1) * 4, 256);
        cond_pool_off = arena.alloc(cond_pool_cap);
    }
    size_t cond_take(size_t bytes) {
        bytes = round_up_sz(bytes, 256);
        if (cond_pool_used + bytes > cond_pool_cap) throw std::runtime_error("conditional embedding pool exhausted");
        const size_t off = cond_pool_off + cond_pool_used;
        cond_pool_used += bytes;
        return off;
    }
    // ce = W2 act(W0 fourier_embedding(param, E) + b0) + b2 for the MLP `mlp`.{i0,i2} (in-major vec packs)
    void emit_cond_base(const std::string& mlp, const char* i0, const char* i2, int E, int Hd, int act, size_t ce_off) {
        const int half = E / 2;
        std::vector<float> fr(half);
        for (int i = 0; i < half; ++i) fr[i] = (float)std::exp(-std::log(10000.0) * (double)((float)i) / (double)half);
        Op op;
        op.type = OP_CONDBASE; op.name = mlp; op.cls = CLS_COND;
        memset(&op.cb, 0, sizeof op.cb);
        op.cb.param = as_ptr<const float>(tag(SP_EXT0 + EX_PARAM, 0)); op.cb.B = B; op.cb.E = E; op.cb.Hd = Hd; op.cb.act = act;
        op.cb.freqs = as_ptr<const float>(const_floats(fr));
        op.cb.w0_t = as_ptr<const float>(vecp(vec_id(mlp + "." + i0 + ".weight")));
        op.cb.b0 = as_ptr<const float>(vecp(vec_id(mlp + "." + i0 + ".bias")));
        op.cb.w2_t = as_ptr<const float>(vecp(vec_id(mlp + "." + i2 + ".weight")));
        op.cb.b2 = as_ptr<const float>(vecp(vec_id(mlp + "." + i2 + ".bias")));
        cond_ce_off = ce_off;
        cond_ce = tag(SP_WS, cond_ce_off); cond_ce_live = true;
        op.cb.ce = as_ptr<float>(cond_ce);
        plan->ops.push_back(op);
    }
    // conditional propagator, step-invariant part: cond_emb_proj(fourier_embedding(param))
    // train_stage2_twophase_conditional.py:116, modules/cond_utils.py:19-38
    void emit_cond_base() {
        const lns_config& c = e->cfg;
        const int E = c.cond_emb_dim;
        emit_cond_base(std::string(c.prop_prefix) + "cond_emb_proj", "0", "2", E, E, ACT_GELU, cond_take((size_t)B * E * 4));
    }

    // CondResidualBlock (norm=True, n_groups=1, GELU, use_scale_shift_norm=False): modules/cond_utils.py:112-128
    //   h = conv1(gelu(GN1(x))) + Linear(cond_emb)[:, :, None, None];  out = conv2(gelu(GN1(h))) + shortcut(x)
    TRef lower_condres(const Layer& l, TRef x, bool raw_out) {
        if (x.pending()) throw std::runtime_error("CondResidualBlock input must be materialised: " + l.name);
        if (!cond_ce_live) throw std::runtime_error("CondResidualBlock without a conditioning embedding: " + l.name);
        const int E = l.cr_E;
        // emb_out = cond_emb(emb): [B, cout], weights in the reference's [out][in] layout
        const size_t emb_off = arena.alloc((size_t)B * l.cout * 4);
        {
            Op op;
            op.type = OP_VECLIN; op.name = l.name + ".cond_emb"; op.cls = CLS_COND;
            op.vl.in = as_ptr<const float>(cond_ce); op.vl.w = as_ptr<const float>(vecp(l.cr_lin_w));
            op.vl.bias = as_ptr<const float>(vecp(l.cr_lin_b)); op.vl.out = as_ptr<float>(tag(SP_WS, emb_off));
            op.vl.B = B; op.vl.In = E; op.vl.Out = l.cout; op.vl.ldi = E; op.vl.ldo = 1;
            plan->ops.push_back(op);
        }
        TRef skip = x;
        bool skip_owned = false;
        if (l.chup >= 0) { skip = conv_same1(x, l.chup, ACT_NONE, nullptr, nullptr, l.name + ".shortcut", -1, false); skip_owned = true; }
        TRef xin = x; xin.owned = false;
        emit_gn(xin, 1, 1e-5f, l.g1, l.b1, 0, l.name + ".norm1");
        TRef a1 = emit_apply(xin, ACT_GELU, l.name + ".act1");          // (the conv prologue knows Swish only)
        free_t(xin);
        TRef h1 = conv_same3(a1, l.conv1, 1, l.mode_y, l.mode_x, ACT_NONE, nullptr, tag(SP_WS, emb_off), l.name + ".conv1", false);
        free_t(a1);
        arena.release(emb_off);
        emit_gn(h1, 1, 1e-5f, l.g2, l.b2, 0, l.name + ".norm2");
        TRef a2 = emit_apply(h1, ACT_GELU, l.name + ".act2");
        free_t(h1);
        TRef out = conv_same3(a2, l.conv2, 1, l.mode_y, l.mode_x, ACT_NONE, &skip, 0, l.name + ".conv2", raw_out);
        free_t(a2);
        if (skip_owned) free_t(skip);
        return out;
    }

    // conditional DilatedResidualBlock: train_stage2_twophase_conditional.py:25-75
    TRef lower_condblock(const Layer& l, TRef x, bool raw_out) {
        const lns_config& c = e->cfg;
        const int D = l.C, E = c.cond_emb_dim;
        const std::string q = l.name;
        const size_t emb_off = cond_take((size_t)B * D * 4), mul_off = cond_take((size_t)B * D * 4);
        {
            Op op;
            op.type = OP_CONDBLK; op.name = q + ".cond"; op.cls = CLS_COND;
            op.ck.ce = as_ptr<const float>(cond_ce); op.ck.B = B; op.ck.E = E; op.ck.D = D;
            op.ck.wce_t = as_ptr<const float>(vecp(vec_id(q + ".cond_emb.weight")));
            op.ck.bce = as_ptr<const float>(vecp(vec_id(q + ".cond_emb.bias")));
            op.ck.gn_g = as_ptr<const float>(vecp(vec_id(q + ".cond_conv2.0.weight")));
            op.ck.gn_b = as_ptr<const float>(vecp(vec_id(q + ".cond_conv2.0.bias")));
            op.ck.c1_t = as_ptr<const float>(vecp(vec_id(q + ".cond_conv2.1.weight")));
            op.ck.c1_b = as_ptr<const float>(vecp(vec_id(q + ".cond_conv2.1.bias")));
            op.ck.c3_t = as_ptr<const float>(vecp(vec_id(q + ".cond_conv2.3.weight")));
            op.ck.c3_b = as_ptr<const float>(vecp(vec_id(q + ".cond_conv2.3.bias")));
            op.ck.emb = as_ptr<float>(tag(SP_WS, emb_off)); op.ck.mul = as_ptr<float>(tag(SP_WS, mul_off));
            plan->ops.push_back(op);
        }
        TRef xin = x; xin.owned = false;
        emit_gn(xin, 1, 1e-5f, l.p_g1, l.p_b1, 0, q + ".conv1.0");
        TRef h1 = conv_same3(xin, l.p_c1, 1, l.mode_y, l.mode_x, ACT_GELU, nullptr, 0, q + ".conv1.1");
        free_t(xin);
        TRef h2 = conv_same3(h1, l.p_c3, l.dil, l.mode_y, l.mode_x, ACT_NONE, nullptr, tag(SP_WS, emb_off), q + ".conv1.3", false);
        free_t(h1);
        emit_gn(h2, 1, 1e-5f, l.c_g, l.c_b, 0, q + ".cond_conv1.0");
        // GroupNorm -> GELU -> conv: the f16x2 3x3 kernel applies both in its prologue (mode 3); any other kernel gets the
        // materialised tensor (round 2's form, LNS_NO_GELU_PROLOGUE=1)
        const bool no_gelu_pro = knobs().no_gelu_prologue || knobs().conv_fp32_mfma;   // (strict-fp32 runs have no split-operand kernels)
        const ConvPack& cpk = e->packs[l.c_conv];
        TRef x1;
        bool fused_gelu = false;
        if (!no_gelu_pro && cpk.has_wb && cpk.f16 && cpk.cout > 32) {
            // the pack is eligible; whether the GEOMETRY picks the f16x2 kernel is only known inside emit_conv
            TRef h2g = h2; h2g.owned = false; h2g.ss_owned = false; h2g.act = ACT_GELU;
            try {
                x1 = conv_same3(h2g, l.c_conv, 1, l.mode_y, l.mode_x, ACT_NONE, &x, 0, q + ".cond_conv1.2", false);
                fused_gelu = true;
            } catch (const NoGeluPrologue&) {}
        }
        if (fused_gelu) {
            free_t(h2);
        } else {
            TRef h3 = emit_apply(h2, ACT_GELU, q + ".cond_conv1.1");
            free_t(h2);
            x1 = conv_same3(h3, l.c_conv, 1, l.mode_y, l.mode_x, ACT_NONE, &x, 0, q + ".cond_conv1.2", false);
            free_t(h3);
        }
        TRef xin2 = x1; xin2.owned = false;
        emit_gn(xin2, 1, 1e-5f, l.p_g2, l.p_b2, tag(SP_WS, mul_off), q + ".ffn.0");
        TRef f1 = conv_same1(xin2, l.p_f1, ACT_GELU, nullptr, nullptr, q + ".ffn.1");
        free_t(xin2);
        TRef out = conv_same1(f1, l.p_f3, ACT_NONE, &x1, nullptr, q + ".ffn.3", -1, raw_out);
        free_t(f1); free_t(x1);
        // emb / mul (and cond_ce) are never released: they depend on `param` only, so the steps after the first one
        // of a rollout reuse them (Runner::skip_step_invariant) and nothing else may be placed there
        return out;
    }

    // FourierBasicBlock: x + gelu(SpectralConv2d(x) + conv1x1(x))   modules/basics.py:574-583
    TRef lower_fourier(const Layer& l, TRef x, const TRef* out_forced, bool raw_out) {
        if (x.pending()) throw std::runtime_error("FourierBasicBlock input must be materialised");
        if (l.cin != x.C || l.cin != l.cout) throw std::runtime_error("FourierBasicBlock needs in == out channels: " + l.name);
        const int C = x.C, H = x.H, W = x.W, m1 = l.m1, m2 = l.m2;
        if (2 * m1 > H || m2 > W / 2 + 1) throw std::runtime_error("too many Fourier modes for this resolution: " + l.name);
        TRef x2 = conv_same1(x, l.f_conv, ACT_NONE, nullptr, nullptr, l.name + ".conv", -1, false);
        TRef x1 = alloc_t(C, H, W);
        const size_t t1 = arena.alloc((size_t)B * C * H * m2 * 2 * 4), xf = arena.alloc((size_t)B * C * 2 * m1 * m2 * 2 * 4),
                     of = arena.alloc((size_t)B * C * 2 * m1 * m2 * 2 * 4);
        {
            Op op;
            op.type = OP_SPECTRAL; op.name = l.name + ".fourier"; op.cls = CLS_SPECTRAL;
            memset(&op.sp, 0, sizeof op.sp);
            op.sp.x = as_ptr<const float>(x.ptr); op.sp.x_bs = x.bs; op.sp.B = B; op.sp.Cin = C; op.sp.Cout = C;
            op.sp.H = H; op.sp.W = W; op.sp.m1 = m1; op.sp.m2 = m2;
            op.sp.w1 = as_ptr<const float>(vecp(l.f_w1)); op.sp.w2 = as_ptr<const float>(vecp(l.f_w2));
            op.sp.t1 = as_ptr<float>(tag(SP_WS, t1)); op.sp.xf = as_ptr<float>(tag(SP_WS, xf));
            op.sp.of = as_ptr<float>(tag(SP_WS, of)); op.sp.y = as_ptr<float>(x1.ptr);
            op.flops = 8.0 * B * C * ((double)H * W * m2 + 2.0 * H * m1 * m2) * 2 + 8.0 * B * C * C * 2.0 * m1 * m2;
            plan->ops.push_back(op);
        }
        arena.release(t1); arena.release(xf); arena.release(of);
        TRef out = out_forced ? *out_forced : alloc_t(C, H, W);
        {
            Op op;
            op.type = OP_FCOMBINE; op.name = l.name + ".combine"; op.cls = CLS_MISC;
            op.fc.a = as_ptr<const float>(x1.ptr); op.fc.b = as_ptr<const float>(x2.ptr); op.fc.e = nullptr;
            op.fc.skip = as_ptr<const float>(x.ptr); op.fc.skip_bs = x.bs; op.fc.y = as_ptr<float>(out.ptr);
            op.fc.y_bs = out.bs; op.fc.B = B; op.fc.C = C; op.fc.HW = H * W; op.fc.act = ACT_GELU;
            out.amax = 0; out.amax_const = 0.0f; out.gn_bound = 0.0f; op.fc.amax_out = nullptr;
            if (raw_out && !out_forced) { out.amax = new_amax(l.name + ".combine"); op.fc.amax_out = as_ptr<unsigned>(out.amax); }
            plan->ops.push_back(op);
        }
        free_t(x1); free_t(x2);
        return out;
    }

    // sequential program ---------------------------------------------------------
    // does layer j read its input un-normalised through a (possibly split-operand) convolution?
    static bool reads_raw(const std::vector<Layer>& L, size_t j) {
        if (j >= L.size()) return false;                       // the program's output
        switch (L[j].type) {
            case LT_CONV: case LT_UP2: case LT_RESIZE: case LT_FOURIER: return true;
            case LT_RES: case LT_CONDRES: return L[j].chup >= 0;
            default: return false;                             // GroupNorm / LayerNorm first (GN, SA, FA, propagator blocks), Swish
        }
    }
    void lower_sequence(const std::vector<Layer>& L, TRef in, const TRef& out_ext) {
        TRef cur = in;
        for (size_t i = 0; i < L.size(); ++i) {
            const Layer& l = L[i];
            const bool last = (i + 1 == L.size());
            const bool raw_next = reads_raw(L, i + 1);
            TRef nxt;
            switch (l.type) {
                case LT_CONV: {
                    int act_out = ACT_NONE;
                    size_t skip = 0;
                    int fuse = -1;
                    int pack = l.pack;
                    // conv -> 1x1 conv with nothing in between: ONE conv on the weights composed at pack time (lns_fold.h),
                    // under the 1x1's layer name like the fused-epilogue form below (the intermediate is not traced there either)
                    const bool folded = e->opt_fold_linear && l.fold >= 0 && !last;
                    if (folded) { pack = l.fold; skip = 1; }
                    const size_t j = i + 1 + skip;                 // the layer behind this conv (or behind the pair)
                    // conv -> Swish with no norm in between: fuse the activation into the epilogue
                    if (j < L.size() && L[j].type == LT_SWISH) { act_out = ACT_SWISH; ++skip; }
                    // conv -> 1x1 conv (64 -> 64): the second conv runs in the first one's epilogue
                    else if (!folded && !last && L[i + 1].type == LT_CONV && L[i + 1].k == 1 && L[i + 1].stride == 1 &&
                             can_fuse_1x1(e->packs[l.pack], e->packs[L[i + 1].pack])) { fuse = L[i + 1].pack; skip = 1; }
                    const bool is_last = (i + 1 + skip == L.size());
                    const std::string& nm = (folded || fuse >= 0) ? L[i + 1].name : l.name;
                    nxt = emit_conv(cur, pack, l.k, l.stride, l.dil, l.pad, l.mode_y, l.mode_x, act_out, nullptr, 0,
                                    is_last ? &out_ext : nullptr, nm, fuse, reads_raw(L, i + 1 + skip));
                    free_t(cur);
                    i += skip;
                    if (!is_last) trace(nm, nxt);
                    break;
                }
                case LT_SWISH:
                    if (cur.ss == 0 || cur.act != ACT_NONE) throw std::runtime_error("unfusable Swish at " + l.name);
                    cur.act = ACT_SWISH;
                    continue;
                case LT_GN:
                    emit_gn(cur, l.groups, l.eps, l.vg, l.vb, 0, l.name);
                    continue;
                case LT_UP2:
                    if (cur.pending()) throw std::runtime_error("resize of a pending tensor");
                    cur.vH = 2 * cur.H; cur.vW = 2 * cur.W; cur.sch = 0.5f; cur.scw = 0.5f;
                    continue;
                case LT_RESIZE:
                    if (cur.pending()) throw std::runtime_error("resize of a pending tensor");
                    if (l.outH != cur.H || l.outW != cur.W) { cur.vH = l.outH; cur.vW = l.outW; cur.sch = 0; cur.scw = 0; }
                    continue;
                case LT_RES: nxt = lower_res(l, cur, raw_next); free_t(cur); trace(l.name, nxt); break;
                case LT_SA: nxt = lower_sa(l, cur, raw_next); free_t(cur); trace(l.name, nxt); break;
                case LT_FA: nxt = lower_fa(l, cur, raw_next); free_t(cur); trace(l.name, nxt); break;
                case LT_PROPBLOCK: nxt = lower_propblock(l, cur, raw_next); free_t(cur); trace(l.name, nxt); break;
                case LT_CONDBLOCK:
                    if (!cond_ce_live) emit_cond_base();
                    nxt = lower_condblock(l, cur, raw_next); free_t(cur); trace(l.name, nxt); break;
                case LT_FOURIER: nxt = lower_fourier(l, cur, nullptr, raw_next); free_t(cur); trace(l.name, nxt); break;
                case LT_CONDRES: nxt = lower_condres(l, cur, raw_next); free_t(cur); trace(l.name, nxt); break;
                default: throw std::runtime_error("layer type not supported by this build: " + l.name);
            }
            if (last && l.type != LT_CONV) throw std::runtime_error("program must end in a convolution");
            cur = nxt;
        }
    }

    void finish() {
        // int constants first, then float constants, in one device blob
        const size_t ibytes = plan->consts_i.size() * 4;
        for (Op& op : plan->ops) for_each_ptr(op, [&](auto*& p) { rebase_const(p, ibytes); });
        plan->arena_bytes = arena.high;
        plan->amax_bytes = (size_t)amax_used * B * LNS_AMAX_SUB * 4;
    }
};

// ---------------------------------------------------------------------------
// weights
// ---------------------------------------------------------------------------
static void release_overlap_objects(lns_engine* e) {
    for (void* ev : e->events) (void)hipEventDestroy(static_cast<hipEvent_t>(ev));
    e->events.clear();
    if (e->side_stream) { (void)hipStreamDestroy(static_cast<hipStream_t>(e->side_stream)); e->side_stream = nullptr; }
    for (hipStream_t st : e->dec_streams) (void)hipStreamDestroy(st);
    e->dec_streams.clear();
}

// Drop the cached encoder / decoder plans (and the propagator's): the next call plans again.  The engine's device is current.
static void drop_plans(lns_engine* e, bool with_propagator) {
    for (auto* m : {&e->enc_plans, &e->dec_plans, &e->prop_plans}) {
        if (m == &e->prop_plans && !with_propagator) continue;
        for (auto& kv : *m) if (kv.second.d_consts) (void)hipFree(kv.second.d_consts);
        m->clear();
    }
}

static int finalize_weights(lns_engine* e, int device) {
    for (const Param& p : e->params)
        if (!p.is_set) { e->err = "weight not set: " + p.key; return LNS_ESTATE; }
    size_t off = 0;
    for (ConvPack& p : e->packs) {
        p.w_off = off; off += round_up_sz((size_t)p.k * p.k * p.Cin_pad * p.Cout_pad, 64);
        p.b_off = off; off += round_up_sz((size_t)p.Cout_pad, 64);
        p.has_wb = (p.k == 3 && p.Cin_pad % 8 == 0 && p.cout > 32) || (p.k == 1 && p.Cin_pad % 32 == 0);
        if (p.has_wb) {
            p.wb_off = off;
            off += round_up_sz((p.k == 3 ? convb_weight_bytes(p.cout, p.Cin_pad) : convb1_weight_bytes(p.cout, p.Cin_pad)) / 4, 64);
        }
        p.has_wu = p.up2 && p.has_wb && p.k == 3 && !knobs().no_up2_phases;       // (A/B knob: the nine-tap gather form everywhere)
        if (p.has_wu) { p.wu_off = off; off += round_up_sz(convu_weight_bytes(p.cout, p.Cin_pad) / 4, 64); }
    }
    for (VecPack& v : e->vecs) { v.off = off; off += round_up_sz(v.count, 64); }
    std::vector<float> host(off, 0.0f);
    // composed packs (lns_fold.h): W' and b' from the two source packs' current host parameters, once per weight load; from
    // here on the array is packed like any other conv's
    std::vector<std::vector<float>> fold_w(e->packs.size()), fold_b(e->packs.size());
    for (size_t i = 0; i < e->packs.size(); ++i) {
        const ConvPack& p = e->packs[i];
        if (p.fold_a < 0) continue;
        const ConvPack& pa = e->packs[p.fold_a];
        const ConvPack& pb = e->packs[p.fold_b];
        auto host_of = [&](const std::string& key) { return key.empty() ? nullptr : e->params[e->pindex.at(key)].host.data(); };
        fold_w[i].resize((size_t)p.cout * p.cin * p.k * p.k);
        fold_b[i].resize((size_t)p.cout);
        fold_conv_1x1(host_of(pa.wkeys[0]), host_of(pa.bkeys[0]), host_of(pb.wkeys[0]), host_of(pb.bkeys[0]), p.k, p.cin, pa.cout,
                      p.cout, fold_w[i].data(), fold_b[i].data());
    }
    // 3x3 convs: two-term fp16 split (f16x2) unless LNS_CONV3_SPLIT=bf16x3; the weight scale is the power of two
    // that brings the largest |w| of the layer just below 2^14
    const bool conv3_f16 = knobs().conv3_split == CONV3_SPLIT_F16X2;
    for (ConvPack& p : e->packs) {
        p.f16 = false; p.wscale = 1.0f;
        const bool want = p.has_wb && ((p.k == 3 && conv3_f16) || (p.k == 1 && convb1_is_f16()));
        if (!want) continue;
        float mx = 0.0f;
        for (const std::string& key : p.wkeys)
            for (float v : e->params[e->pindex.at(key)].host) mx = std::max(mx, fabsf(v));
        if (p.fold_a >= 0) for (float v : fold_w[&p - e->packs.data()]) mx = std::max(mx, fabsf(v));
        if (!(mx > 0.0f) || !std::isfinite(mx)) { if (p.k == 1) p.wscale = 1.0f; continue; }   // all-zero weights: scale 1 (3x3: bf16x3)
        p.f16 = p.k == 3;
        p.wscale = conv_f16_weight_scale(mx);
        p.wscale_up = p.wscale * 0.25f;          // a phase tap sums up to four taps: keep the fp16 high term below 2^14 as well
    }
    for (const ConvPack& p : e->packs) {
        int co = 0;
        const size_t pi = &p - e->packs.data();
        for (size_t i = 0; i < p.couts.size(); ++i) {      // (a composed pack: one slice, its weights in fold_w / fold_b)
            const float* w = p.fold_a >= 0 ? fold_w[pi].data() : e->params[e->pindex.at(p.wkeys[i])].host.data();
            pack_conv_weight(host.data() + p.w_off, w, co, p.couts[i], p.cin, p.k, p.Cin_pad, p.Cout_pad);
            if (p.has_wb && p.k == 3 && !p.f16) convb_pack_weight(host.data() + p.wb_off, w, co, p.couts[i], p.cin, p.Cin_pad);
            if (p.has_wb && p.k == 3 && p.f16) convf_pack_weight(host.data() + p.wb_off, w, co, p.couts[i], p.cin, p.Cin_pad, p.wscale);
            if (p.has_wu && p.f16) convu_pack_weight(host.data() + p.wu_off, w, co, p.couts[i], p.cin, p.Cin_pad, p.wscale_up);
            if (p.has_wb && p.k == 1) convb1_pack_weight(host.data() + p.wb_off, w, co, p.couts[i], p.cin, p.Cin_pad, p.wscale);
            if (p.fold_a >= 0) {
                if (p.has_bias) memcpy(host.data() + p.b_off, fold_b[pi].data(), (size_t)p.cout * 4);
            } else if (!p.bkeys[i].empty()) {
                const Param& b = e->params[e->pindex.at(p.bkeys[i])];
                memcpy(host.data() + p.b_off + co, b.host.data(), (size_t)p.couts[i] * 4);
            }
            co += p.couts[i];
        }
    }
    std::vector<float> composed;
    for (const VecPack& v : e->vecs) {
        const Param& p = e->params[e->pindex.at(v.key)];
        const float* src = p.host.data();
        if (!v.key2.empty()) {
            // composed vector (VecPack::key2): `key` [n][n] applied after `key2` [n][n] is the k = 1, bias-free case of
            // lns_fold.h (compensated double, one rounding) -- from the current host parameters, so a reload recomposes
            const int n = (int)p.shape[0];
            composed.resize(v.count);
            fold_conv_1x1(e->params[e->pindex.at(v.key2)].host.data(), nullptr, p.host.data(), nullptr, 1, n, n, n, composed.data(), nullptr);
            src = composed.data();
        }
        float* dst = host.data() + v.off;
        if (v.xform == VX_NONE) memcpy(dst, src, v.count * 4);
        else if (v.xform == VX_TRANSPOSE2D) transpose_rows(dst, src, (size_t)p.shape[0], v.count / (size_t)p.shape[0]);   // [out][in] -> [in][out]
        else if (v.xform == VX_PE_T) transpose_rows(dst, src, (size_t)p.shape[1], (size_t)p.shape[2]);                    // [1][L][C] -> [C][L]
    }
    HIPCHK(e, hipSetDevice(device));
    HIPCHK(e, init_kernels());
    if (e->device >= 0 && e->device != device) release_overlap_objects(e);   // streams / events belong to the old device
    if (e->d_weights) { (void)hipFree(e->d_weights); e->d_weights = nullptr; }
    HIPCHK(e, hipMalloc(reinterpret_cast<void**>(&e->d_weights), std::max<size_t>(off, 64) * 4));
    HIPCHK(e, hipMemcpy(e->d_weights, host.data(), off * 4, hipMemcpyHostToDevice));
    e->weights_floats = off;
    e->device = device;
    e->finalized = true;
    // plans hold weight offsets only, but rotary tables depend on inv_freq: drop cached plans
    drop_plans(e, true);
    e->ran.clear(); e->ran_ws = nullptr; e->ran_B = 0;     // lns_check_finite has nothing to look at until the next run
    return LNS_OK;
}

// ---------------------------------------------------------------------------
// plans
// ---------------------------------------------------------------------------
static TRef ext_tensor(int slot, int C, int H, int W) {
    TRef t;
    t.ptr = tag(SP_EXT0 + slot, 0); t.bs = -(long)(slot + 1); t.C = C; t.H = H; t.W = W;
    return t;
}

static int upload_consts(lns_engine* e, Plan& p) {
    const size_t ib = p.consts_i.size() * 4, fb = p.consts_f.size() * 4;
    if (ib + fb == 0) return LNS_OK;
    HIPCHK(e, hipMalloc(&p.d_consts, ib + fb));
    if (ib) HIPCHK(e, hipMemcpy(p.d_consts, p.consts_i.data(), ib, hipMemcpyHostToDevice));
    if (fb) HIPCHK(e, hipMemcpy(static_cast<char*>(p.d_consts) + ib, p.consts_f.data(), fb, hipMemcpyHostToDevice));
    return LNS_OK;
}

enum PlanKind { PK_ENC, PK_DEC, PK_PROP };

static int get_plan(lns_engine* e, PlanKind kind, int B, int H, int W, Plan** out) {
    auto& m = kind == PK_ENC ? e->enc_plans : (kind == PK_DEC ? e->dec_plans : e->prop_plans);
    const long key = ((long)B << 32) | ((long)H << 16) | (long)W;
    auto it = m.find(key);
    if (it != m.end()) { *out = &it->second; return LNS_OK; }
    if (!e->finalized) { e->err = "lns_finalize_weights must be called first"; return LNS_ESTATE; }
    const lns_config& c = e->cfg;
    Plan plan;
    plan.B = B; plan.H = H; plan.W = W;
    plan.kind = (int)kind; plan.key = key;
    try {
        Planner pl(e, &plan, B);
        pl.init_stat_scratch();
        pl.init_amax_region();
        if (kind == PK_PROP) pl.init_cond_pool();
        if (kind == PK_ENC) {
            if (e->enc.empty()) throw std::runtime_error("engine has no autoencoder");
            if (c.cond_encoder)   // CondEncoder.forward: cond_emb = embed(fourier_embedding(param, E))  (autoencoder2d_nonsquared.py:128)
                pl.emit_cond_base(std::string(c.ae_prefix) + "encoder.embed", "0", "2", c.cond_emb_channels, c.encoder_channels[0],
                                  ACT_SWISH, pl.arena.alloc((size_t)B * c.cond_emb_channels * 4));
            TRef xin = ext_tensor(EX_IN, c.in_channels, c.Ly, c.Lx);
            // lns_encode_affine (plan key H = 1): the caller's per-(sample, channel) (scale, shift) table is the pending
            // prologue of the input, consumed by the encoder's first convolution (no normalised copy of the frames)
            if (H == 1) {
                if (e->enc[0].type != LT_CONV) throw std::runtime_error("encoder does not start with a convolution");
                xin.ss = tag(SP_EXT0 + EX_SS, 0);
            }
            pl.lower_sequence(e->enc, xin, ext_tensor(EX_OUT, e->lat_C, e->lat_H, e->lat_W));
        } else if (kind == PK_DEC) {
            if (e->dec.empty()) throw std::runtime_error("engine has no autoencoder");
            pl.lower_sequence(e->dec, ext_tensor(EX_IN, e->lat_C, e->lat_H, e->lat_W),
                              ext_tensor(EX_OUT, c.in_channels, c.Ly, c.Lx));
        } else {
            if (e->prop.empty()) throw std::runtime_error("engine has no propagator");
            pl.lower_sequence(e->prop, ext_tensor(EX_IN, c.latent_dim, H, W), ext_tensor(EX_OUT, c.latent_dim, H, W));
        }
        pl.finish();
    } catch (const std::exception& ex) {
        e->err = ex.what();
        return LNS_EINVAL;
    }
    int rc = upload_consts(e, plan);
    if (rc) return rc;
    auto res = m.emplace(key, std::move(plan));
    *out = &res.first->second;
    return LNS_OK;
}

// ---------------------------------------------------------------------------
// execution
// ---------------------------------------------------------------------------
#if defined(LNS_TS) || defined(FAF_TS)
// diagnostic builds: launch(stamps) with a zeroed [blocks][words] stamp buffer, wait for it, and append the header line and one
// "<block> <words ...>" line per block to $LNS_TS_FILE (tools/ts_analyze.py, faf_ts_analyze.py, clock_analyze.py read that).
// false: no file named or no buffer, and nothing was launched
template <class L> static bool ts_capture(long blocks, int words, const std::string& header, hipStream_t s, hipError_t& rc, L&& launch) {
    const char* path = getenv("LNS_TS_FILE");
    const size_t n = (size_t)blocks * words;
    long long* dts = nullptr;
    if (!path || hipMalloc(reinterpret_cast<void**>(&dts), n * 8) != hipSuccess) return false;
    (void)hipMemsetAsync(dts, 0, n * 8, s);
    rc = launch(dts);
    (void)hipStreamSynchronize(s);
    std::vector<long long> h(n);
    (void)hipMemcpy(h.data(), dts, n * 8, hipMemcpyDeviceToHost);
    (void)hipFree(dts);
    if (FILE* f = fopen(path, "a")) {
        fprintf(f, "%s\n", header.c_str());
        for (long i = 0; i < blocks; ++i) {
            fprintf(f, "%ld", i);
            for (int k = 0; k < words; ++k) fprintf(f, " %lld", h[(size_t)i * words + k]);
            fprintf(f, "\n");
        }
        fclose(f);
    }
    return true;
}
#endif

struct EvPair { hipEvent_t a, b; int cls; const Op* op; };

struct Runner {
    lns_engine* e;
    hipStream_t stream;
    std::vector<EvPair> evs;
    Runner(lns_engine* e_, hipStream_t s) : e(e_), stream(s) {}
    // steps > 0 of a rollout: the conditional propagator's embedding MLPs depend on `param` only and their outputs
    // live at fixed, never-reused arena offsets -- skip them
    bool skip_step_invariant = false;

    int run(const Plan& plan, const ExtT* ext, char* arena_base) {
        Bases B = {};
        B.b[SP_WS] = arena_base;
        B.b[SP_WT] = reinterpret_cast<char*>(e->d_weights);
        B.b[SP_CT] = static_cast<char*>(plan.d_consts);
        for (int i = 0; i < EX_COUNT; ++i) {
            B.b[SP_EXT0 + i] = const_cast<char*>(static_cast<const char*>(ext[i].ptr));
            B.bs[SP_EXT0 + i] = ext[i].bs; B.bs2[SP_EXT0 + i] = ext[i].bs2; B.bdiv[SP_EXT0 + i] = ext[i].bdiv;
        }
        // the amax side channel accumulates with atomic max: every run of the plan starts from zero
        // has this (plan, arena) pair already run in this call?  (the first run finds whatever the workspace held before)
        bool seen = false;
        if (e->ran_ws) {
            const size_t off = (size_t)(arena_base - static_cast<const char*>(e->ran_ws));
            for (const auto& r : e->ran) seen = seen || (r.kind == plan.kind && r.key == plan.key && r.arena_off == off);
            if (!seen) e->ran.push_back({plan.kind, plan.key, off});
        }
        if (plan.amax_bytes) {
            // "track_nonfinite": what this region recorded in its PREVIOUS run of this call (an earlier step of the
            // rollout, another decode group) is folded into the engine's sticky word before it is zeroed
            if (e->opt_track_nonfinite && e->d_sticky && seen)
                HIPCHK(e, launch_amax_sticky(reinterpret_cast<const unsigned*>(arena_base + plan.amax_off), (int)(plan.amax_bytes / 4),
                                             e->d_sticky + plan.kind, stream));
            HIPCHK(e, hipMemsetAsync(arena_base + plan.amax_off, 0, plan.amax_bytes, stream));
        }
        for (const Op& op : plan.ops) {
            if (skip_step_invariant && (op.type == OP_CONDBASE || op.type == OP_CONDBLK)) continue;
            EvPair ev;
            if (e->timing_on && op.type != OP_TRACE) {
                HIPCHK(e, hipEventCreate(&ev.a));
                HIPCHK(e, hipEventCreate(&ev.b));
                ev.cls = op.cls; ev.op = &op;
                HIPCHK(e, hipEventRecord(ev.a, stream));
            }
            hipError_t rc = hipSuccess;
#ifdef LNS_DIAG
            // diagnostic build only (make DIAGFLAGS=-DLNS_DIAG; timing what-ifs, results are garbage): LNS_SKIP_OPS=gn,fasmall
            static const char* skip = getenv("LNS_SKIP_OPS");
            if (skip) {
                const bool is_gn = op.type == OP_GNSTATS;
                const bool is_fas = op.type == OP_FAPOOL || op.type == OP_FARED || op.type == OP_FALRK || op.type == OP_FARED2 || op.type == OP_FALRK2 ||
                                    (op.type == OP_CONV && op.name.find("to_qk") != std::string::npos);
                if ((is_gn && strstr(skip, "gn")) || (is_fas && strstr(skip, "fasmall"))) continue;
            }
#endif
            // resolve a copy of the op's block(s), launch only if every pointer resolved (B.bad is reported below)
            auto go = [&](auto a, auto launch) { if (resolve(a, B)) rc = launch(a, stream); };
            auto go2 = [&](auto a, auto b, auto launch) { if (resolve(a, B) && resolve(b, B)) rc = launch(a, b, stream); };   // both axes
            switch (op.type) {
                case OP_CONV: {
                    ConvArgs a = op.conv;
                    if (!resolve_conv(a, B)) break;
#ifdef LNS_TS
                    // diagnostic build: per-block phase timestamps of the layer named by $LNS_TS_LAYER, appended to $LNS_TS_FILE
                    // ($LNS_TS_SKIP: leave the first N launches of the layer alone -- a stamp taken after seconds of sustained load)
                    static long ts_seen = 0;
                    const bool ts_match = getenv("LNS_TS_LAYER") && op.name.find(getenv("LNS_TS_LAYER")) != std::string::npos &&
                                          (cv_is_split_3x3(op.variant) || op.variant == CV_B1);
                    const long ts_skip = getenv("LNS_TS_SKIP") ? atol(getenv("LNS_TS_SKIP")) : 0, ts_max = getenv("LNS_TS_MAX") ? atol(getenv("LNS_TS_MAX")) : (1L << 40);
                    // (the phase forms of the upsampling conv launch four / two blocks per source tile)
                    const long nblk = (long)a.tiles_x * a.tiles_y * a.cout_tiles * a.B * (a.up2 == 1 ? 4 : a.up2 == 4 ? 2 : 1);
                    if (ts_match && ts_seen++ >= ts_skip && ts_seen - 1 - ts_skip < ts_max &&
                        ts_capture(nblk, 8, fmt("# launch %s B=%d Cin=%d Cout=%d H=%d W=%d blocks=%ld", op.name.c_str(), a.B, a.Cin, a.Cout, a.Hout, a.Wout, nblk),
                                   stream, rc, [&](long long* ts) { a.dbg_ts = ts; return launch_conv(op.variant, a, stream); })) break;
#endif
                    rc = launch_conv(op.variant, a, stream);
                    break;
                }
                case OP_GNSTATS: {
                    GnStatsArgs a = op.gn;
                    const float* tp = op.gn_tile_part;
                    if (!resolve(a, B) || !fix(tp, B)) break;
                    if (op.gn_tiles)
                        rc = launch_gn_tile_finalize(a, tp, op.gn_tiles, op.gn_count < 0 ? 0 : (op.gn_count ? op.gn_count : GN_TILE_PIXELS),
                                                     op.gn_geom, stream);
                    else rc = launch_gn_stats(a, a.ss + (size_t)a.B * a.C * 2, stream);
                    break;
                }
                case OP_LNPE: go(op.ln, launch_ln_pe); break;
                case OP_ATTN: go(op.at, launch_attention); break;
                case OP_FAPOOL: go(op.fp, launch_fa_pool); break;
                case OP_FARED: go(op.fr, launch_fa_reducer); break;
                case OP_FARED2: go2(op.fr, op.fr2, launch_fa_reducer2); break;
                case OP_FALRK: go(op.fl, launch_fa_lrk); break;
                case OP_FALRK2: go2(op.fl, op.fl2, launch_fa_lrk2); break;
                case OP_FASAND: go(op.fs, launch_fa_sandwich); break;
                case OP_FAGSPLIT: go(op.fg, launch_fa_gsplit); break;
                case OP_FAFUSED: {
                    FaFusedArgs a = op.ff;
                    if (!resolve(a, B)) break;
                    a.dbg_ts = nullptr;
#ifdef FAF_TS
                    // diagnostic build: wave 0's phase timestamps of every block, appended to $LNS_TS_FILE
                    const long nblk = (long)a.B * a.heads * (a.C / 16 / a.gpb);
                    if (ts_capture(nblk, 24, fmt("# launch %s blocks=%ld", op.name.c_str(), nblk), stream, rc,
                                   [&](long long* ts) { a.dbg_ts = ts; return launch_fa_fused(a, stream); })) break;
#endif
                    rc = launch_fa_fused(a, stream);
                    break;
                }
                case OP_CONDBASE: go(op.cb, launch_cond_base); break;
                case OP_CONDBLK: go(op.ck, launch_cond_block); break;
                case OP_APPLY: go(op.ap, launch_apply); break;
                case OP_SPECTRAL: go(op.sp, launch_spectral); break;
                case OP_FCOMBINE: go(op.fc, launch_fourier_combine); break;
                case OP_VECLIN: go(op.vl, launch_vec_linear); break;
                case OP_TRACE: {
                    if (!e->trace_on) break;
                    const float* p = as_ptr<const float>(op.t_ptr);
                    long bs = op.t_bs;
                    if (!fix(p, B)) break;
                    fixbs(bs, B);
                    HIPCHK(e, hipStreamSynchronize(stream));
                    TraceRec r;
                    r.name = op.name; r.B = plan.B; r.C = op.tC; r.H = op.tH; r.W = op.tW;
                    const size_t per = (size_t)op.tC * op.tH * op.tW;
                    r.data.resize(per * plan.B);
                    for (int b = 0; b < plan.B; ++b)
                        HIPCHK(e, hipMemcpy(r.data.data() + per * b, p + bs * b, per * 4, hipMemcpyDeviceToHost));
                    e->trace.push_back(std::move(r));
                    break;
                }
                default: e->err = "op not implemented: " + op.name; return LNS_EINVAL;
            }
            if (B.bad) {
                e->err = fmt("internal error: unresolved pointer argument in %s (not launched)", op.name.c_str());
                return LNS_EINVAL;
            }
            if (rc != hipSuccess) {
                e->err = fmt("launch of %s failed: %s", op.name.c_str(), hipGetErrorString(rc));
                return LNS_EHIP;
            }
            {   // LNS_DEBUG_SYNC=1 (diagnosis of a device fault): name every launch on stderr and wait for it, so that the last
                // line printed names the kernel that faulted
                if (knobs().debug_sync && op.type != OP_TRACE) {
                    fprintf(stderr, "[lns] %s (plan B=%d, chunk b0=%d nb=%d)\n", op.name.c_str(), plan.B,
                            op.type == OP_CONV ? op.conv.b0 : (op.type == OP_FASAND ? op.fs.b0 : 0),
                            op.type == OP_CONV ? op.conv.B : (op.type == OP_FASAND ? op.fs.B : plan.B));
                    fflush(stderr);
                    const hipError_t se = hipStreamSynchronize(stream);
                    if (se != hipSuccess) { e->err = fmt("%s: %s", op.name.c_str(), hipGetErrorString(se)); return LNS_EHIP; }
                }
            }
            if (e->timing_on && op.type != OP_TRACE) {
                HIPCHK(e, hipEventRecord(ev.b, stream));
                evs.push_back(ev);
            }
        }
        return LNS_OK;
    }

    int finish() {
        if (!e->timing_on || evs.empty()) return LNS_OK;
        HIPCHK(e, hipStreamSynchronize(stream));
        const bool by_name = knobs().timing_by_name;   // per-layer breakdown for profiling
        if (e->timing.empty() && !by_name) {
            e->timing.resize(CLS_COUNT);
            for (int i = 0; i < CLS_COUNT; ++i) e->timing[i].name = kClsName[i];
        }
        if (e->timing_overhead_ms < 0.0) {
            // calibration: a CHAIN of (event, EMPTY launch, event) triples enqueued back to back on the same stream -- the state a
            // timed plan run is in: dispatch latencies overlap the previous launch -- read after one synchronise; the empty
            // kernel itself runs ~1 us
            constexpr int NCAL = 96;
            std::vector<hipEvent_t> ea(NCAL), eb(NCAL);
            int made = 0;
            for (; made < NCAL; ++made)
                if (hipEventCreate(&ea[made]) != hipSuccess || hipEventCreate(&eb[made]) != hipSuccess) break;
            for (int i = 0; i < made; ++i) {
                (void)hipEventRecord(ea[i], stream);
                (void)launch_empty(stream);
                (void)hipEventRecord(eb[i], stream);
            }
            (void)hipStreamSynchronize(stream);
            std::vector<float> v;
            for (int i = 0; i < made; ++i) {
                float ms = 0;
                if (i >= 16 && hipEventElapsedTime(&ms, ea[i], eb[i]) == hipSuccess) v.push_back(ms);     // (the first ones fill the queue)
                (void)hipEventDestroy(ea[i]); (void)hipEventDestroy(eb[i]);
            }
            std::sort(v.begin(), v.end());
            // What is subtracted is 0.6 x that interval: a rocprofv3 dispatch duration (the reference the per-form times are
            // checked against, tools/roofline_from_stats.py) already contains part of the launch ramp an empty launch consists
            // of -- measured: the excess of the event interval over the rocprofv3 duration is 4.6 us per launch where the
            // empty-launch interval is 7.8 us (profiled runs, 11 kernel forms within +-0.6 us; profiles/r04_event_overhead.txt)
            e->timing_overhead_ms = v.empty() ? 0.0 : 0.6 * std::max(0.0, (double)v[v.size() / 2] - 1.0e-3);
        }
        auto named = [&](const std::string& nm) {
            for (TimeRec& r : e->timing) if (r.name == nm) return &r;
            e->timing.emplace_back();
            e->timing.back().name = nm;
            return &e->timing.back();
        };
        for (EvPair& ev : evs) {
            float ms = 0;
            (void)hipEventElapsedTime(&ms, ev.a, ev.b);
            TimeRec* t[2] = {nullptr, nullptr};
            if (!by_name) {
                // per class, and per kernel FORM inside the class ("class/form": nine-tap / four-tap / fp32-MFMA 3x3, ...)
                if (ev.op->form[0]) t[1] = named(std::string(kClsName[ev.cls]) + "/" + ev.op->form);
                t[0] = &e->timing[ev.cls];        // (after named(): emplace_back may move the vector)
            } else t[0] = named(std::string(kClsName[ev.cls]) + ":" + ev.op->name);
            ms = std::max(ms - (float)e->timing_overhead_ms, 0.5e-3f);      // (never below half a microsecond per launch)
            for (TimeRec* r : t)
                if (r) { r->ms += ms; r->launches += 1; r->flops += ev.op->flops; r->bytes += ev.op->bytes; r->mfma_flops += ev.op->mfma_flops; }
            (void)hipEventDestroy(ev.a); (void)hipEventDestroy(ev.b);
        }
        evs.clear();
        return LNS_OK;
    }
};

// What a rollout call does with the latent chain: exactly one of
//   SINK_LATENTS  every latent into `out` [B][T][zper]; nothing is decoded
//   SINK_STEPS    every step decoded into `out` [B][T][xper]
//   SINK_KEPT     the steps keep[0 .. n_keep) decoded into `out` [B][n_keep][xper]; the chain still runs all T steps
//   SINK_SCORED   every step decoded into a frame buffer of the workspace and scored against y_true right there; the frames
//                 of the steps keep[0 .. n_keep) are copied to frames_out
//   SINK_ENSEMBLE the chain runs at batch N = B * M (launch sample b * M + m is member m of trajectory b); the steps
//                 keep[0 .. n_keep) are decoded into a frame buffer of the workspace and reduced over the members right there
//                 into `out` (mean) and `var_out` [B][n_keep][xper]; what else is taken from the frames there: EnsForm
enum SinkKind { SINK_LATENTS, SINK_STEPS, SINK_KEPT, SINK_SCORED, SINK_ENSEMBLE };

// What a SINK_ENSEMBLE call takes from a decoded group beside the mean / variance (lns_rollout_latent_ensemble and its five
// forms): nothing, for which alone `out` is mandatory; the scores against y_true (_eval); the members' quantiles and exceedance
// probabilities (_quantiles); the exceedance tables against y_true (_exceed); the Gram against the observations, then the filter
// (_analysis); the patch Gram, then one transform per latent pixel (_analysis_local).  Under any other sink it means nothing.
enum EnsForm { ENS_STATS, ENS_SCORED, ENS_QUANT, ENS_EXCEED, ENS_ANALYSIS, ENS_ANALYSIS_LOCAL };
static bool ens_analysis(EnsForm f) { return f == ENS_ANALYSIS || f == ENS_ANALYSIS_LOCAL; }

// workspace layout: [ z0 | latent ring: NGROUP groups x kdec steps x [B][zper] | NDEC decode arenas | propagator arena ]
// The propagator gets its own arena because it runs on a second stream, concurrently with decode.
// Step-batched decode: the decodes of different steps are independent given z_t, so the latent chain runs ahead and
// `kdec` consecutive steps are decoded by ONE launch set at batch B * kdec (4x the blocks per launch on the 16x16 /
// 32x32 decoder layers, a quarter of the launches, weight slabs amortised).  A trajectory-step's arithmetic does not
// depend on the batch it rides in (kernel accumulation order is a function of the layer only), so the result is
// bit-identical for every kdec.
// Behind it, from round_up(that layout's total, 256) on, the region the sink needs (kept and frame regions for the ensemble sink):
//   SINK_SCORED  one frame buffer per decode stream (the decode output of a group, [kdec][B][C][Ly][Lx]), then the
//                metric's per-plane sums [B][eval_max_steps][C][2]; a call with time maps appends their state (add_maps_region)
//   SINK_KEPT    two latent buffers [B][zper] that take the latents of the steps nobody decodes
//   SINK_ENSEMBLE  (B = N) the two latent buffers of SINK_KEPT, then the frame buffers of SINK_SCORED
enum { NDEC = 4, NGROUP_MAX = NDEC + 2 };   // max decode streams; latent groups in flight
struct WsLayout {
    size_t z_bytes, ring_off, group_bytes, arena_off, arena_stride, prop_off, total; int ndec, kdec, ngroup;
    size_t fbuf_off, fbuf_stride, part_off;   // SINK_SCORED; SINK_ENSEMBLE (no part)
    size_t pp_off[2];                         // SINK_KEPT, SINK_ENSEMBLE
    size_t maps_off = 0, maps_bytes = 0;      // SINK_SCORED with time maps (add_maps_region)
    size_t etkf_off = 0;                      // SINK_ENSEMBLE, the analysis forms (add_analysis_region)
    // SINK_SCORED with attribution (add_attrib_region): second frame buffers, true-latent staging, three partial-sum arrays
    size_t fbuf2_off = 0, ztrue_off = 0, ztrue_stride = 0, part2_off = 0, ppart_off = 0, lpart_off = 0; long zstride = 0;
};

static int decode_group(const lns_engine* e, int B) {
    // trajectories x steps per decode launch set: about 256 samples ("decode_group" option; 1 = one step per launch)
    int k = e->opt_decode_group > 0 ? e->opt_decode_group : std::max(1, 256 / std::max(1, B));
    k = std::min(k, 8);
    while (k > 1 && (long)B * k > LNS_MAX_BATCH) --k;
    return k;
}

// `total` is what a call with this sink needs.  encode / decode / lns_prepare use the layout of SINK_STEPS; the arena offsets
// lns_check_finite reads back are the same for every sink
static int ws_layout(lns_engine* e, int B, SinkKind sink, WsLayout* L) {
    size_t arena = 0, parena = 0;
    Plan* p;
    int rc;
    L->kdec = decode_group(e, B);
    if (!e->enc.empty()) {
        if ((rc = get_plan(e, PK_ENC, B, 0, 0, &p))) return rc;
        arena = std::max(arena, p->arena_bytes);
        for (int kk = 1; kk <= L->kdec; ++kk) {           // a rollout's last group may hold fewer steps
            if ((rc = get_plan(e, PK_DEC, B * kk, 0, 0, &p))) return rc;
            arena = std::max(arena, p->arena_bytes);
        }
    }
    if (!e->prop.empty() && e->lat_H > 0) {
        if ((rc = get_plan(e, PK_PROP, B, e->lat_H, e->lat_W, &p))) return rc;
        parena = p->arena_bytes;
    }
    const size_t zper = (size_t)std::max(1, e->lat_C) * std::max(1, e->lat_H) * std::max(1, e->lat_W);
    L->z_bytes = round_up_sz((size_t)B * zper * 4, 256);
    L->ndec = std::min((int)NDEC, std::max(1, e->opt_decode_streams));
    L->ngroup = L->ndec + 2;                                           // one being written, one per decode stream, one spare
    L->group_bytes = (size_t)L->kdec * B * zper * 4;                   // steps of a group are contiguous: [kdec][B][zper]
    L->ring_off = L->z_bytes;
    L->arena_off = round_up_sz(L->ring_off + (size_t)L->ngroup * L->group_bytes, 256);
    L->arena_stride = round_up_sz(arena, 256);                        // one decode arena per decode stream
    L->prop_off = L->arena_off + (size_t)L->ndec * L->arena_stride;
    L->total = L->prop_off + round_up_sz(parena, 256) + 256;
    L->fbuf_off = L->fbuf_stride = L->part_off = L->pp_off[0] = L->pp_off[1] = 0;
    if (sink == SINK_KEPT || sink == SINK_ENSEMBLE) {
        L->pp_off[0] = round_up_sz(L->total, 256);
        L->pp_off[1] = L->pp_off[0] + L->z_bytes;                     // (z_bytes is a multiple of 256)
        L->total = L->pp_off[1] + L->z_bytes;
    }
    if (sink == SINK_SCORED || sink == SINK_ENSEMBLE) {
        const size_t xper = (size_t)e->cfg.in_channels * e->cfg.Ly * e->cfg.Lx;
        L->fbuf_off = round_up_sz(L->total, 256);
        L->fbuf_stride = round_up_sz((size_t)L->kdec * B * xper * 4, 256);
        L->total = L->fbuf_off + (size_t)L->ndec * L->fbuf_stride;
    }
    if (sink == SINK_SCORED) {
        L->part_off = L->total;
        L->total = L->part_off + round_up_sz((size_t)B * e->opt_eval_max_steps * e->cfg.in_channels * 2 * 4, 256);
    }
    return LNS_OK;
}

// The state of the time maps (lns_rollout_eval_maps): 52 bytes per (b, c, pixel), behind the SINK_SCORED layout, which it leaves
// byte for byte as it is.
static size_t time_maps_state_bytes(size_t B, size_t C, size_t H, size_t W) {
    return round_up_sz(B * C * H * W * LNS_TIME_MAPS_STATE_PER_PIXEL, 256);
}
static void add_maps_region(const lns_engine* e, int B, WsLayout* L) {
    L->maps_off = round_up_sz(L->total, 256);
    L->maps_bytes = time_maps_state_bytes((size_t)B, (size_t)e->cfg.in_channels, (size_t)e->cfg.Ly, (size_t)e->cfg.Lx);
    L->total = L->maps_off + L->maps_bytes;
}

// The region of the two analysis forms behind the SINK_ENSEMBLE layout, which it leaves byte for byte as it is; offsets from the
// region's start, the *_loc ones for ENS_ANALYSIS_LOCAL only.
struct AnalysisRegion {
    size_t part, S, g, stat, X, wbar, lam, status, S_loc = 0, g_loc = 0, X_loc = 0, wbar_loc = 0, lam_loc = 0, status_loc = 0, bytes = 0;
    size_t take(size_t n) { const size_t at = bytes; bytes = round_up_sz(bytes + n, 256); return at; }   // the next buffer, 256-byte aligned
};
// lns_rollout_latent_ensemble_analysis: the slice partials [B][n_keep][slices][M*M + M + 3], then S [B][n_keep][M][M],
// g [B][n_keep][M], stat [B][n_keep][3], X [B][M][M], wbar [B][M], lam [B][M] (all double) and status [B] (int32)
static AnalysisRegion etkf_region(const lns_engine* e, size_t B, size_t M, size_t n_keep) {
    const size_t nsl = (size_t)etkf_slices((long)e->cfg.in_channels * e->cfg.Ly * e->cfg.Lx), bn = B * n_keep;
    AnalysisRegion r;
    r.part = r.take(bn * nsl * etkf_part_doubles((int)M) * 8);
    r.S = r.take(bn * M * M * 8); r.g = r.take(bn * M * 8); r.stat = r.take(bn * 3 * 8);
    r.X = r.take(B * M * M * 8); r.wbar = r.take(B * M * 8); r.lam = r.take(B * M * 8); r.status = r.take(B * 4);
    return r;
}
// lns_rollout_latent_ensemble_analysis_local: the patch sums [B][n_keep][h*w][M*M + M + 3], then per domain S [B][h*w][M][M],
// g [B][h*w][M], X [B][h*w][M][M], wbar, lam [B][h*w][M], status [B][h*w], then the global S [B][M][M], g [B][M],
// stat [B][n_keep][3], X [B][M][M], wbar [B][M], lam [B][M], status [B]
static AnalysisRegion letkf_region(const lns_engine* e, size_t B, size_t M, size_t n_keep) {
    const size_t hw = (size_t)e->lat_H * e->lat_W, bd = B * hw;
    AnalysisRegion r;
    r.part = r.take(B * n_keep * hw * etkf_part_doubles((int)M) * 8);
    r.S_loc = r.take(bd * M * M * 8); r.g_loc = r.take(bd * M * 8);
    r.X_loc = r.take(bd * M * M * 8); r.wbar_loc = r.take(bd * M * 8); r.lam_loc = r.take(bd * M * 8); r.status_loc = r.take(bd * 4);
    r.S = r.take(B * M * M * 8); r.g = r.take(B * M * 8); r.stat = r.take(B * n_keep * 3 * 8);
    r.X = r.take(B * M * M * 8); r.wbar = r.take(B * M * 8); r.lam = r.take(B * M * 8); r.status = r.take(B * 4);
    return r;
}
static AnalysisRegion analysis_region(const lns_engine* e, EnsForm form, size_t B, size_t M, size_t n_keep) {
    return form == ENS_ANALYSIS_LOCAL ? letkf_region(e, B, M, n_keep) : etkf_region(e, B, M, n_keep);
}
static void add_analysis_region(const lns_engine* e, EnsForm form, int B, int M, int n_keep, WsLayout* L) {
    L->etkf_off = round_up_sz(L->total, 256);
    L->total = L->etkf_off + analysis_region(e, form, B, M, n_keep).bytes;
}

// The region of the error attribution (lns_rollout_eval_attrib), behind the SINK_SCORED layout, which it leaves byte for byte
// as it is: per decode stream a second frame buffer (the reconstruction of the group's truth frames) and a staging buffer
// [kdec][B][zstride] of their latents (zstride: zper rounded up to four floats, so that every slot is 16-byte aligned), then
// the partial sums of the reconstruction [B][eval_max_steps][C][2], (PP, XX, G) [B][eval_max_steps][C][3] and the latent pairs
// [B][eval_max_steps][2].
static void add_attrib_region(const lns_engine* e, int B, WsLayout* L) {
    const size_t zper = (size_t)std::max(1, e->lat_C) * std::max(1, e->lat_H) * std::max(1, e->lat_W);
    const size_t planes = round_up_sz((size_t)B * e->opt_eval_max_steps * e->cfg.in_channels * 2 * 4, 256);
    L->zstride = (long)((zper + 3) / 4 * 4);
    L->fbuf2_off = round_up_sz(L->total, 256);
    L->ztrue_off = L->fbuf2_off + (size_t)L->ndec * L->fbuf_stride;
    L->ztrue_stride = round_up_sz((size_t)L->kdec * B * L->zstride * 4, 256);
    L->part2_off = L->ztrue_off + (size_t)L->ndec * L->ztrue_stride;
    L->ppart_off = L->part2_off + planes;
    L->lpart_off = L->ppart_off + round_up_sz((size_t)B * e->opt_eval_max_steps * e->cfg.in_channels * 3 * 4, 256);
    L->total = L->lpart_off + round_up_sz((size_t)B * e->opt_eval_max_steps * 2 * 4, 256);
}

// An ascending list of steps on the host -- the kept frames, the spectrum steps, the statistics steps of a call -- under
// the name the refusals use, with the cursor of the one walk rollout_loop makes over it
struct StepList {
    const int* steps; int n; const char* name; int next = 0;
    // strictly ascending, in [0, T); the refusal's text into *err
    int check(int T, std::string* err) const {
        for (int i = 0; i < n; ++i)
            if (steps[i] < 0 || steps[i] >= T || (i > 0 && steps[i] <= steps[i - 1])) {
                *err = fmt("%s must be ascending steps in [0, %d): entry %d is %d", name, T, i, steps[i]);
                return LNS_EINVAL;
            }
        return LNS_OK;
    }
    // the entries of the decode group of steps t0g .. t0g + kk - 1 (kk <= 8; ascending: each entry lies in one group),
    // relative to t0g, into sel; returns their number.  The first of them is entry `next` before the call.
    int pick(int t0g, int kk, unsigned char* sel) {
        int m = 0;
        for (; next < n && steps[next] < t0g + kk; ++next) sel[m++] = (unsigned char)(steps[next] - t0g);
        return m;
    }
};

// One rollout call, as the entry points (lns_rollout, lns_rollout_latent, their _eval / _select forms and
// lns_rollout_latent_ensemble) describe it
struct RolloutCall {
    RolloutCall(const float* start_, bool encode_, const float* param_, int B_, int T_, void* ws_, size_t ws_bytes_, void* stream_)
        : start(start_), encode(encode_), param(param_), B(B_), T(T_), ws(ws_), ws_bytes(ws_bytes_), stream(stream_) {}
    const float* start = nullptr; bool encode = false;   // x [B][xper], encoded into z0 first, or the latent z_in [B][zper]
    const float* param = nullptr; int B = 0, T = 0;
    SinkKind sink = SINK_STEPS;
    float* out = nullptr;                                // every sink but SINK_SCORED (SINK_ENSEMBLE: the mean)
    const int* keep = nullptr; int n_keep = 0;           // SINK_KEPT, SINK_ENSEMBLE (n_keep >= 1), SINK_SCORED (n_keep >= 0); host, ascending
    // SINK_ENSEMBLE: B above is the chain's batch N = traj * M (clipped to int; 0 when either factor is not positive)
    int traj = 0, M = 0; float* var_out = nullptr;
    EnsForm ens_form = ENS_STATS;                        // SINK_ENSEMBLE: which of the fields below the call reads
    // ENS_SCORED: y_true [traj][n_keep], spec and seq_out below; the plane sums go straight into scores_out
    float* scores_out = nullptr; int32_t* rank_out = nullptr;
    // ENS_QUANT: qspec, the outputs it asks for, and `spec` below as the nullable denormalisation
    const lns_ensemble_quantile_spec* qspec = nullptr; float *quant_out = nullptr, *prob_out = nullptr;
    // ENS_EXCEED: xspec, y_true [traj][n_keep], the table, and `spec` below as the nullable denormalisation
    const lns_ensemble_exceed_spec* xspec = nullptr; int32_t* table_out = nullptr;
    // ENS_ANALYSIS, ENS_ANALYSIS_LOCAL: y_true [traj][n_keep] holds the observations, rinv their weights with its two strides,
    // `spec` below the nullable denormalisation, rho the inflation; z_analysis and the nullable outputs of the filter
    const float* rinv = nullptr; int64_t rinv_bs = 0, rinv_ss = 0; double rho = 1.0;
    float *z_analysis = nullptr, *param_analysis = nullptr;
    double *X_out = nullptr, *wbar_out = nullptr, *lam_out = nullptr, *stat_out = nullptr; int32_t* status_out = nullptr;
    // ENS_ANALYSIS_LOCAL: the patch Gram takes the Gram's place; the taper's half-width and boundary codes, and the nullable
    // per-domain outputs
    double loc_radius = 0.0; int bc_y = 0, bc_x = 0;
    double *X_loc_out = nullptr, *wbar_loc_out = nullptr, *lam_loc_out = nullptr; int32_t* status_loc_out = nullptr;
    // SINK_SCORED: y_true and the per-plane sums hold T_total steps, of which the call's step 0 is step t0
    const float* y_true = nullptr; int t0 = 0, T_total = 0; const lns_eval_spec* spec = nullptr;
    float *frame_out = nullptr, *seq_out = nullptr, *frames_out = nullptr;
    // SINK_SCORED: the optional selections and their outputs, as include/lns.h states them for lns_eval_select, and which of
    // them the entry form asks for.  spectra: spectra_out [B][n_spec][C][3][S] of the steps spectrum_steps_host (the
    // _spectrum form: always; the others: n_spec != 0); stats: stats_out / hist_out of the steps stats_steps_host (the _stats
    // form: always; _maps: n_stats != 0); maps: maps_out over the steps t >= map_from of the horizon with
    // (t - map_from) % map_every == 0 (the _maps form); sel_bad: that form's lns_eval_select was null or of the wrong size
    lns_eval_select sel = {};
    bool spectra = false, stats = false, maps = false, sel_bad = false;
    // SINK_SCORED: the attribution outputs (the _attrib forms; include/lns.h lns_eval_attrib); at_bad: null or of the wrong size
    lns_eval_attrib at = {};
    bool attrib = false, at_bad = false;
    // SINK_SCORED: the flow diagnostics (the _flow forms; include/lns.h lns_eval_flow) beside the spectra / statistics of `sel`;
    // flow_bad: null or of the wrong size; sel_bad here: a non-null lns_eval_select of the wrong size
    lns_eval_flow fl = {};
    bool flow = false, flow_bad = false;
    StepList flow_list() const { return {fl.flow_steps_host, fl.n_flow, "flow_steps"}; }
    // lns_autoencode_eval: no chain -- x [B][T] is encoded, decoded and scored against itself; only the autoencoder is needed
    bool ae_only = false;
    StepList keep_list() const { return {keep, n_keep, "keep_steps"}; }
    StepList spectrum_list() const { return {sel.spectrum_steps_host, sel.n_spec, "spectrum_steps"}; }
    StepList stats_list() const { return {sel.stats_steps_host, sel.n_stats, "stats_steps"}; }
    float* latents_out = nullptr;                        // optional side outputs: all T latents [B][T][zper],
    float* z_last = nullptr;                             // the latent after the last step [B][zper]
    void* ws = nullptr; size_t ws_bytes = 0; void* stream = nullptr;
};

// second stream + events for the propagate / decode overlap (created once, owned by the engine)
static int ensure_overlap_objects(lns_engine* e) {
    if (e->side_stream) return LNS_OK;
    if (e->opt_prop_priority) {
        int lo = 0, hi = 0;                                   // numerically lower = higher priority
        HIPCHK(e, hipDeviceGetStreamPriorityRange(&lo, &hi));
        HIPCHK(e, hipStreamCreateWithPriority(reinterpret_cast<hipStream_t*>(&e->side_stream), hipStreamNonBlocking, hi));
    } else {
        HIPCHK(e, hipStreamCreateWithFlags(reinterpret_cast<hipStream_t*>(&e->side_stream), hipStreamNonBlocking));
    }
    for (int i = 0; i < NDEC - 1; ++i) {
        hipStream_t st;
        HIPCHK(e, hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        e->dec_streams.push_back(st);
    }
    for (int i = 0; i < 2 * NGROUP_MAX + 1 + 2 * NDEC; ++i) {   // ev_z, ev_free, ev_start, ev_end, ev_maps (rollout_loop)
        hipEvent_t ev;
        HIPCHK(e, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        e->events.push_back(ev);
    }
    return LNS_OK;
}

}  // namespace lns

using namespace lns;

// launches must target the device that holds the packed weights, whatever the caller's current device is
struct DeviceGuard {
    int prev = -1; bool switched = false;
    explicit DeviceGuard(const lns_engine* e) : DeviceGuard(e->device) {}
    explicit DeviceGuard(int device) {
        if (device >= 0 && hipGetDevice(&prev) == hipSuccess && prev != device)
            switched = hipSetDevice(device) == hipSuccess;
    }
    ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
};



// ===========================================================================
// C ABI
// ===========================================================================
extern "C" {

const char* lns_create_error(void) { return g_create_error.c_str(); }

int lns_create(const lns_config* cfg, lns_engine** out) {
    if (!cfg || !out) { g_create_error = "null argument"; return LNS_EINVAL; }
    if (cfg->abi_version != LNS_ABI_VERSION) { g_create_error = "ABI version mismatch"; return LNS_EINVAL; }
    lns_engine* e = new lns_engine();
    e->cfg = *cfg;
    {   // the options' defaults (lns_knobs.h "option default" rows), read at every create
        const OptionDefaults d = option_defaults();
        e->opt_decode_group = (int)d.decode_group;
        e->opt_decode_streams = (int)d.decode_streams;
        e->opt_overlap = d.no_overlap ? 0 : 1;
        e->opt_prop_priority = d.prop_priority ? 1 : 0;
        e->opt_fa_chunk_mb = (int)d.fa_chunk_mb;
        e->opt_fa_fused = (int)std::min(3L, std::max(0L, d.fa_fused));
        e->opt_fa_fused_gpb = (int)std::max(0L, d.fa_fused_gpb);
        e->opt_fold_linear = d.no_fold_linear ? 0 : 1;
        e->opt_up2_dual = d.up2_dual != 0;
    }
    e->cfg.ae_prefix[sizeof(e->cfg.ae_prefix) - 1] = 0;
    e->cfg.prop_prefix[sizeof(e->cfg.prop_prefix) - 1] = 0;
    try {
        build_model(e);
    } catch (const std::exception& ex) {
        g_create_error = ex.what();
        delete e;
        return LNS_EINVAL;
    }
    *out = e;
    return LNS_OK;
}

void lns_train_release(const lns_engine* e);

void lns_destroy(lns_engine* e) {
    if (!e) return;
    lns_train_release(e);
    drop_plans(e, true);
    if (e->d_weights) (void)hipFree(e->d_weights);
    if (e->d_sticky) (void)hipFree(e->d_sticky);
    release_overlap_objects(e);
    delete e;
}

const char* lns_last_error(const lns_engine* e) { return e ? e->err.c_str() : "null engine"; }

int lns_num_params(const lns_engine* e) { return e ? (int)e->params.size() : LNS_EINVAL; }

int lns_param_info(const lns_engine* e, int index, char* key, int key_capacity, int64_t* shape, int* ndim,
                   int* is_buffer) {
    if (!e || index < 0 || index >= (int)e->params.size()) return LNS_EINVAL;
    const Param& p = e->params[index];
    if (key && key_capacity > 0) { strncpy(key, p.key.c_str(), key_capacity - 1); key[key_capacity - 1] = 0; }
    if (shape) for (size_t i = 0; i < p.shape.size() && i < 8; ++i) shape[i] = p.shape[i];
    if (ndim) *ndim = (int)p.shape.size();
    if (is_buffer) *is_buffer = p.is_buffer ? 1 : 0;
    return LNS_OK;
}

int lns_set_weight(lns_engine* e, const char* key, const float* host_data, const int64_t* shape, int ndim) {
    if (!e || !key || !host_data) return LNS_EINVAL;
    auto it = e->pindex.find(key);
    if (it == e->pindex.end()) { e->err = std::string("unexpected key in state_dict: ") + key; return LNS_ENOKEY; }
    Param& p = e->params[it->second];
    if (shape) {
        bool ok = (ndim == (int)p.shape.size());
        for (int i = 0; ok && i < ndim; ++i) ok = (shape[i] == p.shape[i]);
        if (!ok) { e->err = std::string("size mismatch for ") + key; return LNS_ENOKEY; }
    }
    p.host.assign(host_data, host_data + p.numel());
    p.is_set = true;
    e->finalized = false;
    return LNS_OK;
}

int lns_finalize_weights(lns_engine* e, int device) {
    if (!e) return LNS_EINVAL;
    return finalize_weights(e, device);
}

int lns_set_option(lns_engine* e, const char* name, long value) {
    if (!e || !name) return LNS_EINVAL;
    const std::string n = name;
    // a planning rule of the decoder / encoder: cached plans are rebuilt when it changes
    auto set_rule = [e, value](int& opt) { if (opt != (int)value) { DeviceGuard dg(e); drop_plans(e, false); } opt = (int)value; };
    if (n == "decode_group") { if (value < 0 || value > 8) return LNS_EINVAL; e->opt_decode_group = (int)value; }
    else if (n == "decode_streams") { if (value < 1 || value > NDEC) return LNS_EINVAL; e->opt_decode_streams = (int)value; }
    else if (n == "overlap") e->opt_overlap = value != 0;
    else if (n == "eval_max_steps") { if (value < 1 || value > 65536) return LNS_EINVAL; e->opt_eval_max_steps = (int)value; }
    else if (n == "track_nonfinite") e->opt_track_nonfinite = value != 0;
    else if (n == "train_wgrad") {
        if (value != 0 && value != 1) { e->err = "train_wgrad: 0 (one block per output tile) or 1 (batch-parallel)"; return LNS_EINVAL; }
        e->opt_train_wgrad = (int)value;
    }
    else if (n == "spectrum_basis") {
        if (value < 0 || value > 3) { e->err = "spectrum_basis: basis_y | basis_x << 1 with LNS_SPECTRUM_DFT (0) or LNS_SPECTRUM_DCT (1), i.e. 0 .. 3"; return LNS_EINVAL; }
        e->opt_spectrum_basis = (int)value;
        return LNS_OK;                               // it schedules nothing: the records of the last run stay
    }
    else if (n == "fa_fused") { if (value < 0 || value > 3) return LNS_EINVAL; set_rule(e->opt_fa_fused); }
    else if (n == "fa_fused_gpb") { if (value < 0 || value > 64) return LNS_EINVAL; set_rule(e->opt_fa_fused_gpb); }
    else if (n == "fold_linear") {
        if (value != 0 && value != 1) { e->err = "fold_linear: 0 (the pair as it stands) or 1 (one conv on the composed weights)"; return LNS_EINVAL; }
        set_rule(e->opt_fold_linear);
    }
    else if (n == "up2_dual") {
        if (value != 0 && value != 1) { e->err = "up2_dual: 0 (one block per output phase) or 1 (both column phases per block where the form fits)"; return LNS_EINVAL; }
        set_rule(e->opt_up2_dual);
    }
    else if (n == "fa_chunk_mb") { if (value < 0 || value > 4096) return LNS_EINVAL; set_rule(e->opt_fa_chunk_mb); }
    else if (n == "prop_priority") {
        if (e->opt_prop_priority != (value != 0)) { DeviceGuard dg(e); release_overlap_objects(e); }   // recreated with the new priority
        e->opt_prop_priority = value != 0;
    } else { e->err = "unknown option: " + n; return LNS_EINVAL; }
    e->ran.clear(); e->ran_ws = nullptr; e->ran_B = 0;
    return LNS_OK;
}

int lns_latent_shape(const lns_engine* e, int* C, int* H, int* W) {
    if (!e || e->enc.empty()) return LNS_EINVAL;
    if (C) *C = e->lat_C;
    if (H) *H = e->lat_H;
    if (W) *W = e->lat_W;
    return LNS_OK;
}

// the batch is a grid dimension of every kernel (LNS_MAX_BATCH)
static int check_batch(lns_engine* e, int B) {
    if (B > LNS_MAX_BATCH) { e->err = fmt("batch %d exceeds the maximum of %d trajectories per call", B, LNS_MAX_BATCH); return LNS_EINVAL; }
    return LNS_OK;
}

static int einval(lns_engine* e, const char* what) { e->err = what; return LNS_EINVAL; }

static int need_model(lns_engine* e) {
    if (e->enc.empty() || e->prop.empty()) { e->err = "rollout needs autoencoder and propagator"; return LNS_ESTATE; }
    return LNS_OK;
}

// a conditional propagator (and, where the call encodes, a conditional encoder) reads one parameter per trajectory
static int need_param(lns_engine* e, bool encodes, const float* param) {
    if (param) return LNS_OK;
    if (e->cfg.prop_kind == LNS_PROP_CONDITIONAL || (encodes && e->cfg.cond_encoder))
        return einval(e, encodes ? "conditional model needs param" : "conditional propagator needs param");
    return LNS_OK;
}

// the three size queries: the layout's total for the sink (lns_prepare also serves engines that only encode / decode)
static int workspace_bytes(lns_engine* e, int B, SinkKind sink, size_t* bytes) {
    if (!e) return LNS_EINVAL;
    if (B <= 0) return einval(e, "B must be positive");
    if (int brc = check_batch(e, B)) return brc;
    if (sink != SINK_STEPS)
        if (int mrc = need_model(e)) return mrc;
    DeviceGuard dg(e);
    WsLayout L;
    if (int rc = ws_layout(e, B, sink, &L)) return rc;
    if (bytes) *bytes = L.total;
    return LNS_OK;
}

int lns_prepare(lns_engine* e, int B, size_t* bytes) { return workspace_bytes(e, B, SINK_STEPS, bytes); }
int lns_rollout_eval_workspace_bytes(lns_engine* e, int B, size_t* bytes) { return workspace_bytes(e, B, SINK_SCORED, bytes); }
int lns_rollout_select_workspace_bytes(lns_engine* e, int B, size_t* bytes) { return workspace_bytes(e, B, SINK_KEPT, bytes); }

// the chain's batch of an ensemble call: B * M, clipped so that check_batch names the product
static int ensemble_batch(int B, int M) {
    if (B <= 0 || M <= 0) return 0;
    return (int)std::min<long long>((long long)B * M, 0x7fffffffLL);
}
int lns_rollout_ensemble_workspace_bytes(lns_engine* e, int B, int M, size_t* bytes) {
    if (!e) return LNS_EINVAL;
    if (B <= 0) return einval(e, "B must be positive");
    if (M <= 0) return einval(e, "M must be positive");
    return workspace_bytes(e, ensemble_batch(B, M), SINK_ENSEMBLE, bytes);
}

// label: "" / "evaluation " / "selection " / "ensemble " (what the workspace was sized for)
static int check_ws(lns_engine* e, const WsLayout& L, const char* label, void* ws, size_t bytes) {
    if (!ws || bytes < L.total) { e->err = fmt("%sworkspace too small: need %zu bytes, got %zu", label, L.total, bytes); return LNS_ENOMEM; }
    return LNS_OK;
}

// every top-level entry point: forget what the previous call ran (lns_check_finite looks at the LAST call only)
static void begin_run(lns_engine* e, const void* ws, int B) {
    e->ran.clear(); e->ran_ws = ws; e->ran_B = B;
    e->sticky_armed = false;
}
// (called once the stream of the run is known: the sticky word is zeroed IN STREAM ORDER, in front of the run's kernels)
static int arm_sticky(lns_engine* e, hipStream_t s) {
    if (!e->opt_track_nonfinite) return LNS_OK;
    if (!e->d_sticky) HIPCHK(e, hipMalloc(reinterpret_cast<void**>(&e->d_sticky), 16));
    HIPCHK(e, hipMemsetAsync(e->d_sticky, 0, 16, s));
    e->sticky_armed = true;
    return LNS_OK;
}

// encode / decode / propagate: one run of one plan (key B, H, W) on the caller's stream.  The autoencoder's plans run in
// the decode arena of the rollout layout; the propagator on its own needs its plan's arena only, at offset 0 (an engine
// without autoencoder has no layout).
static int run_single(lns_engine* e, PlanKind kind, int B, int H, int W, const ExtT* ext, void* ws, size_t ws_bytes, void* stream) {
    DeviceGuard dg(e);
    Plan* p; int rc; size_t arena_off = 0;
    if (kind == PK_PROP) {
        if ((rc = get_plan(e, kind, B, H, W, &p))) return rc;
        if (!ws || ws_bytes < p->arena_bytes) { e->err = fmt("workspace too small: need %zu bytes", p->arena_bytes); return LNS_ENOMEM; }
    } else {
        WsLayout L;
        if ((rc = ws_layout(e, B, SINK_STEPS, &L)) || (rc = check_ws(e, L, "", ws, ws_bytes)) || (rc = get_plan(e, kind, B, H, W, &p))) return rc;
        arena_off = L.arena_off;
    }
    Runner r(e, static_cast<hipStream_t>(stream));
    begin_run(e, ws, B);
    if ((rc = arm_sticky(e, r.stream)) || (rc = r.run(*p, ext, static_cast<char*>(ws) + arena_off))) return rc;
    return r.finish();
}

static int encode_impl(lns_engine* e, const float* x, const float* param, int B, float* z, void* ws, size_t ws_bytes, void* stream,
                       const float* ss = nullptr) {
    if (!e || !x || !z || B <= 0) return LNS_EINVAL;
    if (int brc = check_batch(e, B)) return brc;
    const lns_config& c = e->cfg;
    ExtT ext[EX_COUNT];
    ext[EX_IN] = {x, (long)c.in_channels * c.Ly * c.Lx};
    ext[EX_OUT] = {z, (long)e->lat_C * e->lat_H * e->lat_W};
    ext[EX_PARAM] = {param, 1};
    ext[EX_SS] = {ss, (long)c.in_channels * 2};
    return run_single(e, PK_ENC, B, ss ? 1 : 0, 0, ext, ws, ws_bytes, stream);
}

int lns_encode(lns_engine* e, const float* x, int B, float* z, void* ws, size_t ws_bytes, void* stream) {
    if (e && e->cfg.cond_encoder) { e->err = "this autoencoder's encoder is conditional: use lns_encode_cond(x, param)"; return LNS_EINVAL; }
    return encode_impl(e, x, nullptr, B, z, ws, ws_bytes, stream);
}

int lns_encode_cond(lns_engine* e, const float* x, const float* param, int B, float* z, void* ws, size_t ws_bytes, void* stream) {
    if (e && !e->cfg.cond_encoder) { e->err = "lns_encode_cond needs cfg.cond_encoder"; return LNS_EINVAL; }
    if (!param) { if (e) e->err = "conditional encoder needs param"; return LNS_EINVAL; }
    return encode_impl(e, x, param, B, z, ws, ws_bytes, stream);
}

int lns_encode_affine(lns_engine* e, const float* x, const float* scale_shift, const float* param, int B, float* z, void* ws,
                      size_t ws_bytes, void* stream) {
    if (!e || !scale_shift) { if (e) e->err = "lns_encode_affine needs the [B][C][2] (scale, shift) table"; return LNS_EINVAL; }
    if ((e->cfg.cond_encoder != 0) != (param != nullptr)) { e->err = "param must be given exactly for a conditional encoder"; return LNS_EINVAL; }
    return encode_impl(e, x, param, B, z, ws, ws_bytes, stream, scale_shift);
}

int lns_decode(lns_engine* e, const float* z, int B, float* y, void* ws, size_t ws_bytes, void* stream) {
    if (!e || !z || !y || B <= 0) return LNS_EINVAL;
    if (int brc = check_batch(e, B)) return brc;
    const lns_config& c = e->cfg;
    ExtT ext[EX_COUNT];
    ext[EX_IN] = {z, (long)e->lat_C * e->lat_H * e->lat_W};
    ext[EX_OUT] = {y, (long)c.in_channels * c.Ly * c.Lx};
    return run_single(e, PK_DEC, B, 0, 0, ext, ws, ws_bytes, stream);
}

int lns_propagate(lns_engine* e, const float* z_in, const float* param, int B, int H, int W, float* z_out, void* ws,
                  size_t ws_bytes, void* stream) {
    if (!e || !z_in || !z_out || B <= 0 || H <= 0 || W <= 0) return LNS_EINVAL;
    if (int brc = check_batch(e, B)) return brc;
    if (int prc = need_param(e, false, param)) return prc;
    ExtT ext[EX_COUNT];
    const long per = (long)e->cfg.latent_dim * H * W;
    ext[EX_IN] = {z_in, per};
    ext[EX_OUT] = {z_out, per};
    ext[EX_PARAM] = {param, 1};
    return run_single(e, PK_PROP, B, H, W, ext, ws, ws_bytes, stream);
}

// The denormalisation of an lns_eval_spec for C channels as every scored kernel takes it: the scalar form and the
// per-channel part (as lns_metric_rel_l2_ch fills it).  The one place the rule is written on the host; its refusal
// (the per-channel form needs C <= 8) is rollout_refusal's and op_spec_refused's.
static void score_norm(const lns_eval_spec* spec, int C, ScoreNorm* out) {
    out->per_channel = spec->per_channel != 0; out->mean = spec->mean; out->sd = spec->std;
    for (int ch = 0; ch < LNS_METRIC_MAX_CH; ++ch) {
        const bool in = ch < C;
        out->spec.mean[ch] = in ? spec->mean_c[ch] : 0.0f;
        out->spec.std[ch] = in ? spec->std_c[ch] : 1.0f;
        out->spec.flags[ch] = in ? spec->flags_c[ch] : 0;
    }
    out->spec.lo = spec->clamp_lo; out->spec.hi = spec->clamp_hi;
}

// the scoring kernel's arguments for a SINK_SCORED call; frames / kk / y_t / p_t are set per decoded group
static void metric_args(const lns_engine* e, const RolloutCall& c, const WsLayout& L, MetricGroupArgs* mp) {
    MetricGroupArgs& m = *mp;
    m.frames = nullptr; m.y = c.y_true; m.part = reinterpret_cast<float*>(static_cast<char*>(c.ws) + L.part_off);
    m.B = c.B; m.C = e->cfg.in_channels; m.H = e->cfg.Ly; m.W = e->cfg.Lx; m.kk = 0;
    m.y_T = c.T_total; m.y_t = 0; m.p_T = c.T_total; m.p_t = 0;
    score_norm(c.spec, m.C, &m.norm);
}

// the spectrum kernel's arguments for a SINK_SCORED call with spectra; frames / n / sel / y_t / o_t are set per decoded group
static void spectrum_args(const lns_engine* e, const RolloutCall& c, SpectrumArgs* sp) {
    SpectrumArgs& s = *sp;
    s.frames = nullptr; s.y = c.y_true; s.out = c.sel.spectra_out;
    s.B = c.B; s.C = e->cfg.in_channels; s.H = e->cfg.Ly; s.W = e->cfg.Lx; s.K = 3;
    s.basis = e->opt_spectrum_basis;                 // read here, as the call is enqueued
    s.S = lns_spectrum::bins(s.H, s.W, s.basis & 1, s.basis >> 1);
    s.n = 0; s.y_T = c.T_total; s.y_t = 0; s.o_T = c.sel.n_spec; s.o_t = 0;
    score_norm(c.spec, s.C, &s.norm);
    memset(s.sel, 0, sizeof s.sel);
}

// The histogram part of FieldStatsArgs from an lns_stats_spec (nullable: no histograms), for C channels.  Returns the
// refusal's text, or null when the description is usable (or absent).  Host only.
static const char* stats_hist_args(const lns_stats_spec* hs, const int32_t* hist_out, int C, FieldStatsArgs* a) {
    a->hist = nullptr; a->nbins = 0;
    for (int ch = 0; ch < LNS_METRIC_MAX_CH; ++ch) { a->hlo[ch] = 0.0f; a->hhi[ch] = 1.0f; a->hscale[ch] = 1.0f; }
    if (hist_out && !hs) return "hist_out needs a histogram description (hspec is null)";
    if (!hs) return nullptr;
    if (hs->size != sizeof(lns_stats_spec)) return "hspec: the size field is not sizeof(lns_stats_spec)";
    if (hs->nbins < 1 || hs->nbins > 256) return "hspec: nbins must be in 1 .. 256";
    for (int ch = 0; ch < C && ch < LNS_METRIC_MAX_CH; ++ch)
        if (!std::isfinite(hs->lo[ch]) || !std::isfinite(hs->hi[ch]) || !(hs->hi[ch] > hs->lo[ch]))
            return "hspec: the edges of every channel must be finite with hi > lo";
    if (C > LNS_METRIC_MAX_CH) return "histograms need in_channels <= 8";
    if (!hist_out) return nullptr;                   // a description without a destination: no histograms
    a->hist = const_cast<int32_t*>(hist_out); a->nbins = hs->nbins;
    for (int ch = 0; ch < C; ++ch) {
        a->hlo[ch] = hs->lo[ch]; a->hhi[ch] = hs->hi[ch];
        const float width = hs->hi[ch] - hs->lo[ch];
        a->hscale[ch] = (float)hs->nbins / width;
    }
    return nullptr;
}

// the statistics kernel's arguments for a SINK_SCORED call with statistics; frames / n / sel / y_t / o_t are set per decoded group
static void field_stats_args(const lns_engine* e, const RolloutCall& c, FieldStatsArgs* fp) {
    FieldStatsArgs& f = *fp;
    memset(&f, 0, sizeof f);
    f.y = c.y_true; f.stats = c.sel.stats_out;
    f.B = c.B; f.C = e->cfg.in_channels; f.H = e->cfg.Ly; f.W = e->cfg.Lx;
    f.y_T = c.T_total; f.o_T = c.sel.n_stats; f.eps = c.spec->eps;
    score_norm(c.spec, f.C, &f.norm);
    stats_hist_args(c.sel.hspec, c.sel.hist_out, f.C, &f);   // (accepted by rollout_refusal)
}

// The refusals of an lns_flow_spec for C channels and of a histogram destination, in the order of include/lns.h.  Returns
// the refusal's text, or null when the description is usable.  Host only.
static const char* flow_spec_refusal(const lns_flow_spec* fs, int C, const int32_t* hist_out) {
    if (!fs || fs->size != sizeof(lns_flow_spec)) return "fspec is null or its size field is not sizeof(lns_flow_spec)";
    if (fs->cu == fs->cv || fs->cu < 0 || fs->cu >= C || fs->cv < 0 || fs->cv >= C)
        return "fspec: cu and cv must be two different channels of the fields";
    if ((fs->bc_y != LNS_FLOW_PERIODIC && fs->bc_y != LNS_FLOW_WALL) || (fs->bc_x != LNS_FLOW_PERIODIC && fs->bc_x != LNS_FLOW_WALL))
        return "fspec: bc_y and bc_x must be LNS_FLOW_PERIODIC (0) or LNS_FLOW_WALL (1)";
    if (!std::isfinite(fs->dx) || !std::isfinite(fs->dy) || !(fs->dx > 0.0f) || !(fs->dy > 0.0f))
        return "fspec: dx and dy must be finite and positive";
    if (fs->nbins < 0 || fs->nbins > 256) return "fspec: nbins must be in 0 .. 256";
    if (fs->nbins > 0 && (!std::isfinite(fs->lo) || !std::isfinite(fs->hi) || !(fs->hi > fs->lo)))
        return "fspec: the edges must be finite with hi > lo";
    if (hist_out && fs->nbins == 0) return "hist_out needs fspec->nbins > 0";
    return nullptr;
}

// the refusals of the flow part of a scored call, in the order of include/lns.h
static const char* flow_refusal(const RolloutCall& c, int C, std::string* err) {
    if (c.flow_bad) return "flow is null or its size field is not sizeof(lns_eval_flow)";
    if (!c.fl.flow_out) return "flow_out is null";
    if (c.fl.n_flow < 1) return "n_flow must be at least 1";
    if (!c.fl.flow_steps_host) return "flow_steps is null";
    if (c.flow_list().check(c.T, err)) return err->c_str();
    if (const char* why = flow_spec_refusal(c.fl.fspec, C, c.fl.hist_out)) return why;
    if (c.fl.vort_frames_out && c.n_keep == 0) return "vort_frames_out needs n_keep > 0";
    return nullptr;
}

// The flow kernels' arguments from an accepted lns_flow_spec (flow_spec_refusal) and the denormalisation, for [C][H][W] frames;
// the pointers, n and the step bookkeeping are the caller's
static void flow_args(const lns_flow_spec* fs, const lns_eval_spec* spec, int B, int C, int H, int W, FlowStatsArgs* fp) {
    FlowStatsArgs& f = *fp;
    memset(&f, 0, sizeof f);
    f.B = B; f.C = C; f.H = H; f.W = W;
    f.cu = fs->cu; f.cv = fs->cv; f.bc_y = fs->bc_y; f.bc_x = fs->bc_x;
    f.rcy = (float)(1.0 / (2.0 * (double)fs->dy)); f.rey = (float)(1.0 / (double)fs->dy);
    f.rcx = (float)(1.0 / (2.0 * (double)fs->dx)); f.rex = (float)(1.0 / (double)fs->dx);
    f.eps = spec->eps;
    f.nbins = fs->nbins; f.hlo = 0.0f; f.hhi = 1.0f; f.hscale = 1.0f;
    if (fs->nbins > 0) {
        f.hlo = fs->lo; f.hhi = fs->hi;
        const float width = fs->hi - fs->lo;
        f.hscale = (float)fs->nbins / width;
    }
    score_norm(spec, C, &f.norm);
}

// the accumulation kernel's arguments for a SINK_SCORED call with time maps; frames / n / sel / y_t are set per decoded group
static void time_maps_args(const lns_engine* e, const RolloutCall& c, const WsLayout& L, TimeMapsArgs* tp) {
    TimeMapsArgs& t = *tp;
    memset(&t, 0, sizeof t);
    t.y = c.y_true; t.state = static_cast<char*>(c.ws) + L.maps_off; t.maps = c.sel.maps_out;
    t.B = c.B; t.C = e->cfg.in_channels; t.H = e->cfg.Ly; t.W = e->cfg.Lx;
    t.y_T = c.T_total; t.first = c.sel.map_from; t.every = c.sel.map_every;
    t.count = (c.T_total - 1 - c.sel.map_from) / c.sel.map_every + 1;
    score_norm(c.spec, t.C, &t.norm);
}

// The position of probability p among M sorted members (include/lns.h): h = p (M - 1) in double, lo = floor(h), frac = (float)(h - lo)
static void quantile_position(double p, int M, int* lo, float* frac) {
    const double h = p * (double)(M - 1);
    int l = (int)std::floor(h);
    float f = (float)(h - (double)l);
    if (l >= M - 1) { l = M - 1; f = 0.0f; }
    *lo = l; *frac = f;
}

// the refusals of a lns_ensemble_quantile_spec and its outputs, in the order of include/lns.h; nullptr: accepted
static const char* quantile_spec_refusal(const lns_ensemble_quantile_spec* qs, const float* quant_out, const float* prob_out) {
    if (!qs || qs->size != sizeof(lns_ensemble_quantile_spec)) return "qspec is null or its size field is not sizeof(lns_ensemble_quantile_spec)";
    if (qs->n_q < 0 || qs->n_q > LNS_QUANTILE_MAX || qs->n_thr < 0 || qs->n_thr > LNS_QUANTILE_MAX || (qs->n_q == 0 && qs->n_thr == 0))
        return "qspec: n_q and n_thr must be in 0 .. 8 and not both 0";
    for (int k = 0; k < qs->n_q; ++k)
        if (!(qs->q[k] >= 0.0 && qs->q[k] <= 1.0)) return "qspec: every probability must be in [0, 1]";
    if (qs->n_q > 0 && !quant_out) return "quant_out is null but n_q > 0";
    if (qs->n_thr > 0 && !prob_out) return "prob_out is null but n_thr > 0";
    return nullptr;
}

// the quantile kernel's arguments (an accepted qspec; norm nullable); frames / kk / o_T / o_t are the caller's
static void quantile_args(const lns_ensemble_quantile_spec* qs, const lns_eval_spec* norm, int B, int M, int C, int H, int W,
                          float* quant_out, float* prob_out, EnsembleQuantileArgs* qp) {
    EnsembleQuantileArgs& q = *qp;
    memset(&q, 0, sizeof q);
    q.quant = quant_out; q.prob = prob_out;
    q.B = B; q.M = M; q.C = C; q.H = H; q.W = W; q.n_q = qs->n_q; q.n_thr = qs->n_thr;
    q.denorm = norm != nullptr;
    if (norm) score_norm(norm, C, &q.norm);
    for (int k = 0; k < qs->n_q; ++k) quantile_position(qs->q[k], M, &q.lo[k], &q.frac[k]);
    for (int k = 0; k < qs->n_thr; ++k)
        for (int ch = 0; ch < LNS_METRIC_MAX_CH; ++ch) q.thr[k][ch] = qs->thr[k][ch];
}

// the refusals of a lns_ensemble_exceed_spec and its output, in the order of include/lns.h; nullptr: accepted
static const char* exceed_spec_refusal(const lns_ensemble_exceed_spec* xs, const int32_t* table_out) {
    if (!xs || xs->size != sizeof(lns_ensemble_exceed_spec)) return "xspec is null or its size field is not sizeof(lns_ensemble_exceed_spec)";
    if (xs->n_thr < 1 || xs->n_thr > LNS_EXCEED_MAX) return "xspec: n_thr must be in 1 .. 8";
    if (!table_out) return "table_out is null";
    return nullptr;
}

// the exceedance kernel's arguments (an accepted xspec; norm nullable); frames / kk / y_T / y_t / o_T / o_t are the caller's
static void exceed_args(const lns_ensemble_exceed_spec* xs, const lns_eval_spec* norm, const float* y, int B, int M, int C, int H, int W,
                        int32_t* table_out, EnsembleExceedArgs* xp) {
    EnsembleExceedArgs& x = *xp;
    memset(&x, 0, sizeof x);
    x.y = y; x.table = table_out;
    x.B = B; x.M = M; x.C = C; x.H = H; x.W = W; x.n_thr = xs->n_thr;
    x.denorm = norm != nullptr;
    if (norm) score_norm(norm, C, &x.norm);
    for (int k = 0; k < xs->n_thr; ++k)
        for (int ch = 0; ch < LNS_METRIC_MAX_CH; ++ch) x.thr[k][ch] = xs->thr[k][ch];
}

// bytes of an exceedance table [B][n][n_thr][C][2][M + 1]
static size_t exceed_table_bytes(int B, int n, int n_thr, int C, int M) {
    return (size_t)B * n * n_thr * C * 2 * (M + 1) * sizeof(int32_t);
}

// the refusals of the ensemble transform Kalman filter's member count and inflation (include/lns.h); nullptr: accepted
static_assert(LNS_ETKF_MAX_MEMBERS == 64, "the header's LNS_ETKF_MAX_MEMBERS, the messages below and the kernels' LDS budgets say 64");
static const char* etkf_members_refusal(int M) {
    return M < 2 || M > LNS_ETKF_MAX_MEMBERS ? "M in 2 .. 64 (the transform keeps A and Q in LDS; 65 .. 128 members are not supported)" : nullptr;
}
static const char* etkf_rho_refusal(double rho) {
    return !(rho >= 1.0) || std::isinf(rho) ? "rho (the multiplicative inflation) must be finite and >= 1" : nullptr;
}

// the Gram kernel's arguments (norm nullable); frames / part / kk / y_T / y_t / o_T / o_t are the caller's
static void obs_gram_args(const lns_eval_spec* norm, const float* y, const float* rinv, int64_t r_bs, int64_t r_ss, int B, int M, int C,
                          int H, int W, EnsembleObsGramArgs* gp) {
    EnsembleObsGramArgs& g = *gp;
    memset(&g, 0, sizeof g);
    g.y = y; g.rinv = rinv; g.r_bs = (long)r_bs; g.r_ss = (long)r_ss;
    g.B = B; g.M = M; g.C = C; g.H = H; g.W = W; g.nsl = etkf_slices((long)C * H * W);
    g.denorm = norm != nullptr;
    if (norm) score_norm(norm, C, &g.norm);
}

// the refusals of the localised filter's taper (include/lns.h); nullptr: accepted
static const char* letkf_radius_refusal(double radius) {
    return !(radius > 0.0) || std::isinf(radius) ? "loc_radius must be finite and > 0" : nullptr;
}
static const char* letkf_bc_refusal(int bc_y, int bc_x) {
    return (bc_y != LNS_FLOW_PERIODIC && bc_y != LNS_FLOW_WALL) || (bc_x != LNS_FLOW_PERIODIC && bc_x != LNS_FLOW_WALL)
               ? "bc_y / bc_x must be LNS_FLOW_PERIODIC or LNS_FLOW_WALL" : nullptr;
}

// the patch Gram kernel's arguments (norm nullable); frames / part / kk / y_T / y_t / o_T / o_t are the caller's
static void patch_gram_args(const lns_eval_spec* norm, const float* y, const float* rinv, int64_t r_bs, int64_t r_ss, int B, int M, int C,
                            int H, int W, int h, int w, LetkfPatchGramArgs* gp) {
    LetkfPatchGramArgs& g = *gp;
    memset(&g, 0, sizeof g);
    g.y = y; g.rinv = rinv; g.r_bs = (long)r_bs; g.r_ss = (long)r_ss;
    g.B = B; g.M = M; g.C = C; g.H = H; g.W = W; g.h = h; g.w = w;
    g.denorm = norm != nullptr;
    if (norm) score_norm(norm, C, &g.norm);
}

// What a SINK_ENSEMBLE call launches on a decoded group ahead of the mean / variance: the one kernel of the call's form and
// its arguments.  prepare fills them once per call; launch takes the group -- fb [kk][traj][M][xper], the kept steps
// i0 .. i0 + kk - 1 of y_true / y_obs and of the outputs [traj][n_keep] -- and enqueues the kernel.
struct EnsGroup {
    EnsForm form = ENS_STATS;
    union { EnsembleScoreArgs sc; EnsembleQuantileArgs qa; EnsembleExceedArgs xa; EnsembleObsGramArgs oa; LetkfPatchGramArgs pga; };
    void prepare(const lns_engine* e, const RolloutCall& c, const WsLayout& L) {
        const int C = e->cfg.in_channels, H = e->cfg.Ly, W = e->cfg.Lx;
        form = c.ens_form;
        // the analysis forms: the sums of kept step i land in the region's part[b][i]
        double* part = ens_analysis(form) ? reinterpret_cast<double*>(static_cast<char*>(c.ws) + L.etkf_off +
                                                                      analysis_region(e, form, c.traj, c.M, c.n_keep).part) : nullptr;
        switch (form) {
        case ENS_STATS: break;
        case ENS_SCORED:
            sc.frames = nullptr; sc.y = c.y_true; sc.scores = c.scores_out; sc.rank = c.rank_out; sc.pixel = nullptr;
            sc.B = c.traj; sc.M = c.M; sc.C = C; sc.H = H; sc.W = W; sc.kk = 0; sc.y_T = c.n_keep; sc.y_t = 0;
            score_norm(c.spec, C, &sc.norm); break;
        case ENS_QUANT: quantile_args(c.qspec, c.spec, c.traj, c.M, C, H, W, c.quant_out, c.prob_out, &qa); qa.o_T = c.n_keep; break;
        case ENS_EXCEED: exceed_args(c.xspec, c.spec, c.y_true, c.traj, c.M, C, H, W, c.table_out, &xa); xa.y_T = xa.o_T = c.n_keep; break;
        case ENS_ANALYSIS:
            obs_gram_args(c.spec, c.y_true, c.rinv, c.rinv_bs, c.rinv_ss, c.traj, c.M, C, H, W, &oa);
            oa.part = part; oa.y_T = oa.o_T = c.n_keep; break;
        case ENS_ANALYSIS_LOCAL:
            patch_gram_args(c.spec, c.y_true, c.rinv, c.rinv_bs, c.rinv_ss, c.traj, c.M, C, H, W, e->lat_H, e->lat_W, &pga);
            pga.part = part; pga.y_T = pga.o_T = c.n_keep; break;
        }
    }
    hipError_t launch(const float* fb, int kk, int i0, hipStream_t s) {
        switch (form) {
        case ENS_STATS: break;
        case ENS_SCORED: sc.frames = fb; sc.kk = kk; sc.y_t = i0; return launch_ensemble_score(sc, s);
        case ENS_QUANT: qa.frames = fb; qa.kk = kk; qa.o_t = i0; return launch_ensemble_quantile(qa, s);
        case ENS_EXCEED: xa.frames = fb; xa.kk = kk; xa.y_t = xa.o_t = i0; return launch_ensemble_exceed(xa, s);   // counts added into table_out
        case ENS_ANALYSIS: oa.frames = fb; oa.kk = kk; oa.y_t = oa.o_t = i0; return launch_ensemble_obs_gram(oa, s);
        case ENS_ANALYSIS_LOCAL: pga.frames = fb; pga.kk = kk; pga.y_t = pga.o_t = i0; return launch_letkf_patch_gram(pga, s);
        }
        return hipSuccess;
    }
};

// the autoregressive loop of every rollout call: zcur -> T x (propagate ; what the sink does)   (train_stage2_ns2d.py:147-156)
// The latent chain z_t -> z_{t+1} is strictly sequential, but decode(z_t) depends on z_t only: the chain runs ahead
// (on the engine's side stream when overlapping; own arena) writing groups of `kdec` consecutive decoded latents into
// the ring, and every finished group is decoded by one launch set at batch B * kdec on one of the decode streams
// (round-robin, one arena each), ordered by events, so the small latent-resolution kernels of later steps overlap
// the large decode kernels of earlier ones.
// SINK_SCORED: the decode of a group writes that decode stream's frame buffer instead of `out`, the scoring kernel and
// the copies of the kept steps follow on the same decode stream -- in stream order before the next decode that reuses
// the buffer, so the event scheme is the rollout's own.
// SINK_KEPT: the chain still runs all T steps, the decoder runs for the kept ones only.
// SINK_ENSEMBLE: SINK_KEPT at batch N = B * M whose decode writes the decode stream's frame buffer as SINK_SCORED's does;
// the reduction over the members follows on the same decode stream and writes mean / var of out[b][i0 + j].
// SINK_LATENTS: no step is decoded, so there is no group, no side stream and no event: every step is "a step nobody
// decodes", whose latent goes straight into `out` on the caller's stream.
static int rollout_loop(lns_engine* e, Runner& r, ExtT zcur, const RolloutCall& c, const WsLayout& L) {
    Plan* pp;
    int rc;
    const int B = c.B, T = c.T;
    if ((rc = get_plan(e, PK_PROP, B, e->lat_H, e->lat_W, &pp))) return rc;
    const long zper = (long)e->lat_C * e->lat_H * e->lat_W;
    const long xper = (long)e->cfg.in_channels * e->cfg.Ly * e->cfg.Lx;
    const bool scored = c.sink == SINK_SCORED, ens = c.sink == SINK_ENSEMBLE, kept = c.sink == SINK_KEPT || ens;
    const bool latents = c.sink == SINK_LATENTS;
    char* base = static_cast<char*>(c.ws);
    char* arena = base + L.arena_off;
    char* parena = base + L.prop_off;
    hipStream_t stream = r.stream;
    ExtT ext[EX_COUNT];
    ext[EX_PARAM] = {c.param, 1};
    const bool overlap = !latents && !e->trace_on && !e->timing_on && e->opt_overlap;
    const int kdec = e->trace_on ? 1 : L.kdec, ngroup = L.ngroup, ndec = overlap ? L.ndec : 1;
    if (overlap && (rc = ensure_overlap_objects(e))) return rc;
    hipStream_t pstream = overlap ? static_cast<hipStream_t>(e->side_stream) : stream;
    hipStream_t dstream[NDEC];
    char* darena[NDEC];
    std::vector<Runner> rd;
    for (int d = 0; d < ndec; ++d) {
        dstream[d] = d == 0 ? stream : e->dec_streams[d - 1];
        darena[d] = arena + (size_t)d * L.arena_stride;
        if (overlap) rd.emplace_back(e, dstream[d]);
    }
    Runner rp_side(e, pstream);
    Runner& rp = overlap ? rp_side : r;              // single-stream: everything through the caller's runner (timing events)
    hipEvent_t *ev_z = nullptr, *ev_free = nullptr, *ev_end = nullptr, *ev_maps = nullptr;
    if (overlap) {
        ev_z = e->events.data();                     // ev_z[g]: the latents of ring group g are complete
        ev_free = e->events.data() + NGROUP_MAX;     // ev_free[g]: the decode that read ring group g has finished
        hipEvent_t ev_start = e->events[2 * NGROUP_MAX];
        ev_end = e->events.data() + 2 * NGROUP_MAX + 1;   // [0]: propagator stream, [d]: decode stream d
        ev_maps = ev_end + NDEC;                     // [d]: the last time-map accumulation launched on decode stream d
        HIPCHK(e, hipEventRecord(ev_start, stream));
        HIPCHK(e, hipStreamWaitEvent(pstream, ev_start, 0));
        for (int d = 1; d < ndec; ++d) HIPCHK(e, hipStreamWaitEvent(dstream[d], ev_start, 0));
    }
    char* ring = base + L.ring_off;
    std::vector<char> used(ngroup, 0);
    MetricGroupArgs m;
    if (scored) metric_args(e, c, L, &m);
    EnsGroup eg;
    if (ens) eg.prepare(e, c, L);
    SpectrumArgs sx;
    if (scored && c.spectra) spectrum_args(e, c, &sx);
    FieldStatsArgs fs;
    if (scored && c.stats) field_stats_args(e, c, &fs);
    FlowStatsArgs fw, fv;                            // the flow statistics of the selected steps, the vorticity of the kept ones
    if (scored && c.flow) {
        flow_args(c.fl.fspec, c.spec, B, e->cfg.in_channels, e->cfg.Ly, e->cfg.Lx, &fw);
        fv = fw;
        fw.y = c.y_true; fw.stats = c.fl.flow_out; fw.hist = c.fl.hist_out; fw.y_T = c.T_total; fw.o_T = c.fl.n_flow;
        fv.vort = c.fl.vort_frames_out; fv.o_T = c.n_keep;
    }
    TimeMapsArgs tm;
    if (scored && c.maps) time_maps_args(e, c, L, &tm);
    int maps_d = -1;                                 // the decode stream of the latest time-map accumulation of this call
    // attribution: the encoder plan of the truth frames, the reconstruction's metric arguments, (PP, XX) and the latent pairs
    const bool attrib = scored && c.attrib;
    Plan* penc = nullptr;
    MetricGroupArgs m2;
    AttribGroupArgs ag;
    LatentErrArgs la;
    if (attrib) {
        if ((rc = get_plan(e, PK_ENC, B, 0, 0, &penc))) return rc;
        m2 = m; m2.part = reinterpret_cast<float*>(base + L.part2_off);
        ag.frames = ag.recon = nullptr; ag.y = c.y_true; ag.part = reinterpret_cast<float*>(base + L.ppart_off);
        ag.B = B; ag.C = m.C; ag.H = m.H; ag.W = m.W; ag.kk = 0; ag.y_T = c.T_total; ag.y_t = 0; ag.p_T = c.T_total; ag.p_t = 0;
        ag.norm = m.norm;
        la.z = la.ztrue = nullptr; la.part = reinterpret_cast<float*>(base + L.lpart_off);
        la.zstride = L.zstride; la.zper = (int)zper; la.B = B; la.kk = 0; la.T_total = c.T_total; la.t = 0;
        la.mean = 0.0f; la.sd = 1.0f;
    }
    // A decode group is the next up to kdec DECODED steps: all steps, the kept ones, or none.  The chain writes the
    // latent of a decoded step into the group's next ring slot; the latent of a step nobody decodes goes into `out`
    // (SINK_LATENTS) or into the two ping-pong buffers in turn (SINK_KEPT, SINK_ENSEMBLE), so a step never writes the buffer it reads.
    const int n_dec = latents ? 0 : (kept ? c.n_keep : T);   // decoded steps; a decoded `out` is [B][n_dec]
    auto dec_step = [&](int i) { return kept ? c.keep[i] : i; };
    int npp = 0;                                     // the ping-pong buffer the next skipped step writes
    auto chain_step = [&](int t, const ExtT& znext) -> int {   // strictly sequential in t, independent in b
        ext[EX_IN] = zcur;
        ext[EX_OUT] = znext;
        rp.skip_step_invariant = t > 0 && !e->trace_on;
        const int src = rp.run(*pp, ext, parena);
        rp.skip_step_invariant = false;
        if (src) return src;
        if (c.latents_out)
            HIPCHK(e, hipMemcpy2DAsync(c.latents_out + (long)t * zper, (size_t)T * zper * 4, znext.ptr, (size_t)znext.bs * 4,
                                       (size_t)zper * 4, B, hipMemcpyDeviceToDevice, pstream));
        zcur = znext;
        return LNS_OK;
    };
    auto undecoded_step = [&](int t) -> int {
        if (latents) return chain_step(t, ExtT{c.out + (long)t * zper, (long)T * zper});
        const ExtT znext = {base + L.pp_off[npp], zper};
        npp ^= 1;
        return chain_step(t, znext);
    };
    int g = 0, gi = 0, t = 0;                        // t: next step of the chain
    StepList frames_kept = c.keep_list(), spec_steps = c.spectrum_list(), stats_steps = c.stats_list();   // SINK_SCORED: walked group by group
    StepList flow_steps = c.flow_list();
    for (int i0 = 0; i0 < n_dec;) {                  // i0: index in `out` of the group's first step
        const int kk = std::min(kdec, n_dec - i0);
        const int t0g = dec_step(i0);                // the group's first step
        char* gbase = ring + (size_t)g * L.group_bytes;
        // WAR: the decode of the group that lived here (under selection it may have been filled many chain steps ago)
        if (overlap && used[g]) HIPCHK(e, hipStreamWaitEvent(pstream, ev_free[g], 0));
        for (int j = 0; j < kk; ++t) {
            if (t != dec_step(i0 + j)) { if ((rc = undecoded_step(t))) return rc; continue; }
            const ExtT znext = {gbase + (size_t)j * B * zper * 4, zper};
            if ((rc = chain_step(t, znext))) return rc;
            ++j;
        }
        // decode the group: launch sample s = j * B + b reads latent [j][b] and writes out[b][i0 + j]
        Plan* pd;
        if ((rc = get_plan(e, PK_DEC, B * kk, 0, 0, &pd))) return rc;
        const int d = gi % ndec;
        Runner& rdec = overlap ? rd[d] : r;
        float* zt = attrib ? reinterpret_cast<float*>(base + L.ztrue_off + (size_t)d * L.ztrue_stride) : nullptr;
        if (attrib) {
            // Truth encode: y_true[:, t0 + t0g + j] -> zt[j], read in place through the batch stride T_total * xper (every op
            // that reads a plan's input takes its batch stride from the ExtT).  It does not depend on the chain, so it stands
            // ahead of the wait on ev_z[g]; darena[d] and zt are this decode stream's own (stream order covers their reuse).
            ExtT xe[EX_COUNT];
            xe[EX_PARAM] = {c.param, 1};
            for (int j = 0; j < kk; ++j) {
                xe[EX_IN] = {c.y_true + (long)(c.t0 + t0g + j) * xper, (long)c.T_total * xper};
                xe[EX_OUT] = {zt + (long)j * B * L.zstride, L.zstride};
                if ((rc = rdec.run(*penc, xe, darena[d]))) return rc;
                if (c.at.z_true_out)
                    HIPCHK(e, hipMemcpy2DAsync(c.at.z_true_out + (long)(c.t0 + t0g + j) * zper, (size_t)c.T_total * zper * 4,
                                               zt + (long)j * B * L.zstride, (size_t)L.zstride * 4, (size_t)zper * 4, B,
                                               hipMemcpyDeviceToDevice, dstream[d]));
            }
        }
        if (overlap) {
            HIPCHK(e, hipEventRecord(ev_z[g], pstream));
            HIPCHK(e, hipStreamWaitEvent(dstream[d], ev_z[g], 0));
        }
        if (attrib) {                                // latent drift: ring group g against the staged true latents
            la.z = reinterpret_cast<const float*>(gbase); la.ztrue = zt; la.kk = kk; la.t = c.t0 + t0g;
            HIPCHK(e, launch_latent_err_group(la, dstream[d]));
        }
        ext[EX_IN] = {gbase, zper};
        float* fb = scored || ens ? reinterpret_cast<float*>(base + L.fbuf_off + (size_t)d * L.fbuf_stride) : nullptr;
        if (fb) ext[EX_OUT] = {fb, xper};            // [kk][B][xper]: launch sample s = j * B + b
        else ext[EX_OUT] = {c.out + (long)i0 * xper, (long)n_dec * xper, xper, B};
        if ((rc = (overlap ? rd[d] : r).run(*pd, ext, darena[d]))) return rc;
        if (scored) {                                // (every step is decoded: t0g == i0)
            m.frames = fb; m.kk = kk; m.y_t = c.t0 + t0g; m.p_t = c.t0 + t0g;
            HIPCHK(e, launch_metric_group(m, dstream[d]));
            unsigned char kj[8];
            const int ki = frames_kept.next, nk = frames_kept.pick(t0g, kk, kj);
            for (int i = 0; i < nk; ++i)
                HIPCHK(e, hipMemcpy2DAsync(c.frames_out + (long)(ki + i) * xper, (size_t)c.n_keep * xper * 4,
                                           fb + (long)kj[i] * B * xper, (size_t)xper * 4, (size_t)xper * 4, B,
                                           hipMemcpyDeviceToDevice, dstream[d]));
            if (c.spectra) {                         // the group's selected steps, one launch; none: no launch
                sx.frames = fb; sx.y_t = c.t0 + t0g; sx.o_t = spec_steps.next; sx.n = spec_steps.pick(t0g, kk, sx.sel);
                if (sx.n) HIPCHK(e, launch_spectrum_group(sx, dstream[d]));
            }
            if (c.stats) {                           // likewise, beside the spectrum launch
                fs.frames = fb; fs.y_t = c.t0 + t0g; fs.o_t = stats_steps.next; fs.n = stats_steps.pick(t0g, kk, fs.sel);
                if (fs.n) HIPCHK(e, launch_field_stats_group(fs, dstream[d]));
            }
            if (c.flow) {                            // behind the statistics launch; the frame buffer is reused in stream order
                fw.frames = fb; fw.y_t = c.t0 + t0g; fw.o_t = flow_steps.next; fw.n = flow_steps.pick(t0g, kk, fw.sel);
                if (fw.n) HIPCHK(e, launch_flow_stats_group(fw, dstream[d]));
                if (fv.vort && nk) {                 // the vorticity of the group's kept steps, beside their copies
                    fv.frames = fb; fv.o_t = ki; fv.n = nk;
                    for (int i = 0; i < nk; ++i) fv.sel[i] = kj[i];
                    HIPCHK(e, launch_vorticity_group(fv, dstream[d]));
                }
            }
            if (c.maps) {
                // The one result of the scored path that is reduced across groups: a pixel's sums take its steps in ascending
                // order, so the accumulations form a chain across the decode streams -- this one waits for the previous
                // group's, which ran on another stream.  Only the accumulation is chained; decode and scoring stay unordered
                // against other groups.  Last in the group's launches: stream order still covers the frame buffer's reuse.
                tm.frames = fb; tm.y_t = c.t0 + t0g; tm.n = 0;
                for (int j = 0; j < kk; ++j) {
                    const int ta = c.t0 + t0g + j;   // the step of the horizon
                    if (ta >= c.sel.map_from && (ta - c.sel.map_from) % c.sel.map_every == 0) tm.sel[tm.n++] = (unsigned char)j;
                }
                if (tm.n) {
                    if (overlap && maps_d >= 0 && maps_d != d) HIPCHK(e, hipStreamWaitEvent(dstream[d], ev_maps[maps_d], 0));
                    HIPCHK(e, launch_time_maps_group(tm, dstream[d]));
                    if (overlap && ndec > 1) HIPCHK(e, hipEventRecord(ev_maps[d], dstream[d]));
                    maps_d = d;
                }
            }
            if (attrib) {
                // Reconstruction: the group's true latents (the ring group's layout) through the same decode plan into the
                // second frame buffer; the metric's group kernel gives (RR, G), the attribution kernel (PP, XX) from both buffers.
                float* fb2 = reinterpret_cast<float*>(base + L.fbuf2_off + (size_t)d * L.fbuf_stride);
                ExtT xr[EX_COUNT];
                xr[EX_PARAM] = {c.param, 1};
                xr[EX_IN] = {zt, L.zstride};
                xr[EX_OUT] = {fb2, xper};
                if ((rc = rdec.run(*pd, xr, darena[d]))) return rc;
                m2.frames = fb2; m2.kk = kk; m2.y_t = c.t0 + t0g; m2.p_t = c.t0 + t0g;
                HIPCHK(e, launch_metric_group(m2, dstream[d]));
                ag.frames = fb; ag.recon = fb2; ag.kk = kk; ag.y_t = c.t0 + t0g; ag.p_t = c.t0 + t0g;
                HIPCHK(e, launch_attrib_group(ag, dstream[d]));
                if (c.at.recon_frames_out)
                    for (int i = 0; i < nk; ++i)
                        HIPCHK(e, hipMemcpy2DAsync(c.at.recon_frames_out + (long)(ki + i) * xper, (size_t)c.n_keep * xper * 4,
                                                   fb2 + (long)kj[i] * B * xper, (size_t)xper * 4, (size_t)xper * 4, B,
                                                   hipMemcpyDeviceToDevice, dstream[d]));
            }
        }
        if (ens) HIPCHK(e, eg.launch(fb, kk, i0, dstream[d]));   // the form's kernel first, then the mean / variance
        if (ens && c.out) {                       // fb is [kk][traj][M][xper] -> mean / var of out[b][i0 .. i0 + kk)
            EnsembleStatsArgs es;
            es.frames = fb; es.mean = c.out + (long)i0 * xper; es.var = c.var_out ? c.var_out + (long)i0 * xper : nullptr;
            es.per = xper; es.out_bs = (long)n_dec * xper; es.B = c.traj; es.M = c.M; es.kk = kk;
            HIPCHK(e, launch_ensemble_stats(es, dstream[d]));
        }
        if (overlap) { HIPCHK(e, hipEventRecord(ev_free[g], dstream[d])); used[g] = 1; }
        i0 += kk;
        g = (g + 1) % ngroup;
        ++gi;
    }
    for (; t < T; ++t)                               // the steps behind the last decoded one
        if ((rc = undecoded_step(t))) return rc;
    if (c.z_last)   // the last latent is complete once the propagator stream has passed its step
        HIPCHK(e, hipMemcpy2DAsync(c.z_last, (size_t)zper * 4, zcur.ptr, (size_t)zcur.bs * 4, (size_t)zper * 4, B,
                                   hipMemcpyDeviceToDevice, pstream));
    if (overlap) {   // join: everything the side streams did is ordered before whatever the caller enqueues next
        HIPCHK(e, hipEventRecord(ev_end[0], pstream));
        HIPCHK(e, hipStreamWaitEvent(stream, ev_end[0], 0));
        for (int d = 1; d < ndec; ++d) {
            HIPCHK(e, hipEventRecord(ev_end[d], dstream[d]));
            HIPCHK(e, hipStreamWaitEvent(stream, ev_end[d], 0));
        }
    }
    return LNS_OK;
}

// The refusals of a SINK_ENSEMBLE call in two parts, because B / M / T are checked between them (rollout_refusal).  Each check
// stands once, under the forms that have it; the order within a form is part of the interface.  The forms are not uniform: the
// scored form's `spec` is mandatory and refused later under its own text; the exceedance form has no per-channel norm check --
// with more than 8 channels it answers for the thresholds whatever the norm says.
static int analysis_members_refusal(lns_engine* e, int M) {
    const char* why = etkf_members_refusal(M);
    if (why) e->err = std::string("ensemble analysis needs ") + why;
    return why ? LNS_EINVAL : LNS_OK;
}
// part one: the pointers and descriptors of the form
static int ensemble_args_refusal(lns_engine* e, const RolloutCall& c) {
    const EnsForm f = c.ens_form;
    const char* why = nullptr;
    if (ens_analysis(f)) {
        if (!c.y_true) return einval(e, "y_obs is null");
        if (!c.rinv) return einval(e, "rinv is null");
        if (!c.z_analysis) return einval(e, "z_analysis is null");
        if (c.rinv_bs < 0 || c.rinv_ss < 0) return einval(e, "the strides of rinv must be >= 0 (0: shared)");
        if ((why = etkf_rho_refusal(c.rho))) return einval(e, why);
        if (f == ENS_ANALYSIS_LOCAL && (why = letkf_radius_refusal(c.loc_radius))) return einval(e, why);
        if (f == ENS_ANALYSIS_LOCAL && (why = letkf_bc_refusal(c.bc_y, c.bc_x))) return einval(e, why);
    }
    if ((f == ENS_SCORED || f == ENS_EXCEED) && !c.y_true) return einval(e, "y_true is null");
    if (f == ENS_SCORED && !c.scores_out) return einval(e, "scores_out is null");
    if (f == ENS_QUANT && (why = quantile_spec_refusal(c.qspec, c.quant_out, c.prob_out))) return einval(e, why);
    if (f == ENS_EXCEED && (why = exceed_spec_refusal(c.xspec, c.table_out))) return einval(e, why);
    if (f == ENS_STATS && !c.out) return einval(e, "mean_out is null");
    return LNS_OK;
}
// part two, behind B / M / T: the member count, then what the form asks of var_out, param and the nullable norm (`spec`)
static int ensemble_members_refusal(lns_engine* e, const RolloutCall& c) {
    const EnsForm f = c.ens_form;
    const bool wide = e->cfg.in_channels > LNS_METRIC_MAX_CH;
    if (c.var_out && c.M < 2) return einval(e, "var_out needs M >= 2");
    if (f == ENS_SCORED && (c.M < 2 || c.M > LNS_SCORE_MAX_MEMBERS)) return einval(e, "ensemble scoring needs M in 2 .. 128");
    if (f == ENS_QUANT && c.M > LNS_SCORE_MAX_MEMBERS) return einval(e, "ensemble quantiles need M in 1 .. 128");
    if (f == ENS_EXCEED && c.M > LNS_SCORE_MAX_MEMBERS) return einval(e, "ensemble exceedance needs M in 1 .. 128");
    if (ens_analysis(f))
        if (int mrc = analysis_members_refusal(e, c.M)) return mrc;
    if (c.var_out && !c.out) return einval(e, "var_out needs mean_out");         // (ENS_STATS: `out` is not null here)
    if (ens_analysis(f) && c.param_analysis && !c.param) return einval(e, "param_analysis needs param");
    if (f == ENS_STATS || f == ENS_SCORED) return LNS_OK;                         // no nullable norm
    if (c.spec && c.spec->size != sizeof(lns_eval_spec)) return einval(e, "norm: the size field is not sizeof(lns_eval_spec)");
    if (f != ENS_EXCEED && c.spec && c.spec->per_channel && wide) return einval(e, "norm: the per-channel form needs in_channels <= 8");
    if ((f == ENS_EXCEED || (f == ENS_QUANT && c.qspec->n_thr > 0)) && wide) return einval(e, "thresholds need in_channels <= 8");
    if (f == ENS_ANALYSIS_LOCAL && (long)e->lat_H * e->lat_W > LNS_LETKF_MAX_DOMAINS)
        return einval(e, "local ensemble analysis needs a latent grid of at most 4096 pixels");
    return LNS_OK;
}

// every refusal of a rollout call that needs no plan: nothing here touches the device.  The order is part of the
// interface (which of two failing checks answers): arguments, batch, eval_max_steps, the model, param.
static int rollout_refusal(lns_engine* e, const RolloutCall& c) {
    const bool scored = c.sink == SINK_SCORED, ens = c.sink == SINK_ENSEMBLE, kept = c.sink == SINK_KEPT || ens;
    const bool spec_scored = scored || (ens && c.ens_form == ENS_SCORED);   // `spec` is the mandatory one of the scored calls
    if (!c.start) return einval(e, c.encode ? "x is null" : "z_in is null");
    if (int arc = ens ? ensemble_args_refusal(e, c) : LNS_OK) return arc;
    if (scored && !c.y_true) return einval(e, "y_true is null");
    if (!scored && !ens && !c.out) return einval(e, "out is null");
    if ((ens ? c.traj : c.B) <= 0) return einval(e, "B must be positive");
    if (ens && c.M <= 0) return einval(e, "M must be positive");
    if (c.T <= 0) return einval(e, "T must be positive");
    if (int mrc = ens ? ensemble_members_refusal(e, c) : LNS_OK) return mrc;
    if (scored) {
        if (c.t0 < 0 || (long)c.t0 + c.T > c.T_total) {
            e->err = fmt("t0 + T = %d + %d exceeds T_total = %d (or t0 < 0)", c.t0, c.T, c.T_total);
            return LNS_EINVAL;
        }
        if (!c.frame_out && !c.seq_out) return einval(e, "frame_out and seq_out are both null");
    }
    if (spec_scored) {
        if (!c.spec || c.spec->size != sizeof(lns_eval_spec)) return einval(e, "spec is null or its size field is not sizeof(lns_eval_spec)");
        if (c.spec->per_channel && e->cfg.in_channels > LNS_METRIC_MAX_CH) return einval(e, "spec: the per-channel form needs in_channels <= 8");
    }
    if (scored && c.n_keep < 0) return einval(e, "n_keep is negative");
    if (kept && c.n_keep < 1) return einval(e, "n_keep must be at least 1 (for no decoded step: lns_rollout with to_x = 0)");
    if ((scored || kept) && c.n_keep > 0) {
        if (!c.keep) return einval(e, scored ? "keep_steps is null but n_keep > 0" : "keep_steps is null");
        if (scored && !c.frames_out) return einval(e, "frames_out is null but n_keep > 0");
        if (int krc = c.keep_list().check(c.T, &e->err)) return krc;
    }
    if (scored && c.spectra) {
        if (!c.sel.spectra_out) return einval(e, "spectra_out is null");
        if (c.sel.n_spec < 1) return einval(e, "n_spec must be at least 1");
        if (!c.sel.spectrum_steps_host) return einval(e, "spectrum_steps is null");
        if (int src = c.spectrum_list().check(c.T, &e->err)) return src;
        if (!lns_spectrum::supported(e->cfg.Ly, e->cfg.Lx)) {
            e->err = fmt("energy spectrum: a %d x %d plane is not supported (H, W <= 192 and H * W <= 18432)", e->cfg.Ly, e->cfg.Lx);
            return LNS_EINVAL;
        }
    }
    if (scored && c.stats) {
        if (!c.sel.stats_out) return einval(e, "stats_out is null");
        if (c.sel.n_stats < 1) return einval(e, "n_stats must be at least 1");
        if (!c.sel.stats_steps_host) return einval(e, "stats_steps is null");
        if (int src = c.stats_list().check(c.T, &e->err)) return src;
        FieldStatsArgs probe;
        if (const char* why = stats_hist_args(c.sel.hspec, c.sel.hist_out, e->cfg.in_channels, &probe)) return einval(e, why);
    }
    if (scored && c.maps) {
        if (c.sel_bad) return einval(e, "sel is null or its size field is not sizeof(lns_eval_select)");
        if (!c.sel.maps_out) return einval(e, "maps_out is null");
        if (c.sel.map_every < 1) return einval(e, "map_every must be at least 1");
        if (c.sel.map_from < 0 || c.sel.map_from >= c.T_total) {
            e->err = fmt("map_from must be a step in [0, %d), got %d", c.T_total, c.sel.map_from);
            return LNS_EINVAL;
        }
    }
    if (scored && c.attrib) {
        if (c.at_bad) return einval(e, "attrib is null or its size field is not sizeof(lns_eval_attrib)");
        const lns_eval_attrib& a = c.at;
        if (!a.recon_frame && !a.recon_seq && !a.prop_frame && !a.prop_seq && !a.cross_frame && !a.cross_seq && !a.latent_frame &&
            !a.latent_seq && !a.z_true_out && !a.recon_frames_out)
            return einval(e, "attrib: no output is set");
    }
    if (scored && c.flow) {
        if (c.sel_bad) return einval(e, "sel: the size field is not sizeof(lns_eval_select)");
        if (c.sel.maps_out || c.sel.map_from != 0 || c.sel.map_every != 0)
            return einval(e, "sel asks for time maps: the flow form keeps the workspace of lns_rollout_eval (lns_rollout_eval_maps has them)");
        std::string steps_err;
        if (const char* why = flow_refusal(c, e->cfg.in_channels, &steps_err)) return einval(e, why);
    }
    if (int brc = check_batch(e, c.B)) return brc;
    if (scored && c.T_total > e->opt_eval_max_steps) {
        e->err = fmt("%d steps exceed the option eval_max_steps = %d (it sizes the evaluation workspace)", c.T_total, e->opt_eval_max_steps);
        return LNS_EINVAL;
    }
    if (c.ae_only) {                                 // lns_autoencode_eval: the autoencoder alone, param for its encoder alone
        if (e->enc.empty()) { e->err = "autoencode_eval needs an autoencoder"; return LNS_ESTATE; }
        if (e->cfg.cond_encoder && !c.param) return einval(e, "conditional encoder needs param");
        return LNS_OK;
    }
    if (int mrc = need_model(e)) return mrc;
    if (int prc = need_param(e, c.encode, c.param)) return prc;
    if (scored && c.attrib && e->cfg.cond_encoder && !c.param) return einval(e, "conditional encoder needs param");
    return LNS_OK;
}

// whose workspace check_ws finds too small
static const char* ws_label(SinkKind sink, EnsForm form) {
    if (sink == SINK_ENSEMBLE) return form == ENS_ANALYSIS_LOCAL ? "local ensemble analysis " : (form == ENS_ANALYSIS ? "ensemble analysis " : "ensemble ");
    return sink == SINK_SCORED ? "evaluation " : (sink == SINK_KEPT ? "selection " : "");
}

// What a SINK_ENSEMBLE call enqueues on the caller's stream ahead of rollout_loop.  Exceedance tables: the kernels of every decode
// stream add into table_out, so it is cleared on the stream they all start behind (the loop's fork event follows this memset).
static int ensemble_begin(lns_engine* e, const RolloutCall& c, hipStream_t stream) {
    if (c.ens_form == ENS_EXCEED)
        HIPCHK(e, hipMemsetAsync(c.table_out, 0, exceed_table_bytes(c.traj, c.n_keep, c.xspec->n_thr, e->cfg.in_channels, c.M), stream));
    return LNS_OK;
}

// ... and behind it, on the caller's stream once the decode streams have joined.  Scores: the plane sums in scores_out -> the
// scores, in place.  The two filters: the sums of every decode stream and the copy of the last latents (c.z_last: the caller's
// buffer or z_analysis itself) are ordered before them; every buffer has one writer and is read behind it in stream order.
// Global: slice partials -> S, g, stat; the transform; z_last under X.  Local: patch sums -> the tapered (S, g) per domain and
// the global ones; the transform per domain, then the global one; latent pixel l under X_loc[l].  Both: a per-member param under X.
static int ensemble_finish(lns_engine* e, const RolloutCall& c, const WsLayout& L, hipStream_t stream) {
    const int C = e->cfg.in_channels, HW = e->cfg.Ly * e->cfg.Lx, hw = e->lat_H * e->lat_W;
    if (c.ens_form == ENS_SCORED) HIPCHK(e, launch_ensemble_score_finish(c.scores_out, c.traj, c.n_keep, C, HW, c.spec->eps, c.seq_out, stream));
    if (!ens_analysis(c.ens_form)) return LNS_OK;
    const bool local = c.ens_form == ENS_ANALYSIS_LOCAL;
    const AnalysisRegion R = analysis_region(e, c.ens_form, c.traj, c.M, c.n_keep);
    char* rb = static_cast<char*>(c.ws) + L.etkf_off;
    auto dbl = [&](size_t off, double* given = nullptr) { return given ? given : reinterpret_cast<double*>(rb + off); };   // the caller's buffer, or the region's
    auto i32 = [&](size_t off, int32_t* given) { return given ? given : reinterpret_cast<int*>(rb + off); };
    double* stat = dbl(R.stat, c.stat_out);
    // the global transform: of the Grams of the n_keep steps (the transform sums them), or of the one sum combine has made
    const EtkfTransformArgs tg = {dbl(R.S), dbl(R.g), dbl(R.X, c.X_out), dbl(R.wbar, c.wbar_out), dbl(R.lam, c.lam_out), i32(R.status, c.status_out),
                                  c.rho, c.traj, local ? 1 : c.n_keep, c.M};
    if (local) {
        const LetkfCombineArgs ca = {dbl(R.part), dbl(R.S_loc), dbl(R.g_loc), dbl(R.S), dbl(R.g), stat, c.loc_radius, c.traj, c.n_keep, c.M,
                                     e->lat_H, e->lat_W, c.bc_y, c.bc_x};
        const EtkfTransformArgs tl = {ca.S_loc, ca.g_loc, dbl(R.X_loc, c.X_loc_out), dbl(R.wbar_loc, c.wbar_loc_out), dbl(R.lam_loc, c.lam_loc_out),
                                      i32(R.status_loc, c.status_loc_out), c.rho, c.traj * hw, 1, c.M};
        const LetkfUpdateArgs ua = {c.z_last, tl.X, c.z_analysis, c.traj, c.M, e->lat_C, hw};
        HIPCHK(e, launch_letkf_combine(ca, stream));
        HIPCHK(e, launch_etkf_transform(tl, stream));
        HIPCHK(e, launch_etkf_transform(tg, stream));
        HIPCHK(e, launch_letkf_update(ua, stream));
    } else {
        HIPCHK(e, launch_ensemble_obs_gram_finish(dbl(R.part), c.traj * c.n_keep, etkf_slices((long)C * HW), c.M, dbl(R.S), dbl(R.g), stat, stream));
        HIPCHK(e, launch_etkf_transform(tg, stream));
        HIPCHK(e, launch_ensemble_transform(c.z_last, tg.X, c.traj, c.M, (long)e->lat_C * hw, c.z_analysis, stream));
    }
    if (c.param && c.param_analysis) HIPCHK(e, launch_ensemble_transform(c.param, tg.X, c.traj, c.M, 1, c.param_analysis, stream));
    return LNS_OK;
}

// the one call path behind the rollout entry points
static int rollout_call(lns_engine* e, const RolloutCall& c) {
    if (!e) return LNS_EINVAL;
    int rc;
    if ((rc = rollout_refusal(e, c))) return rc;
    const bool scored = c.sink == SINK_SCORED;
    DeviceGuard dg(e);
    WsLayout L;
    if ((rc = ws_layout(e, c.B, c.sink, &L))) return rc;
    if (scored && c.maps) add_maps_region(e, c.B, &L);
    if (scored && c.attrib) add_attrib_region(e, c.B, &L);
    const bool ens = c.sink == SINK_ENSEMBLE;
    if (ens && ens_analysis(c.ens_form)) add_analysis_region(e, c.ens_form, c.traj, c.M, c.n_keep, &L);
    if ((rc = check_ws(e, L, ws_label(c.sink, c.ens_form), c.ws, c.ws_bytes))) return rc;
    Plan* pe = nullptr;
    if (c.encode && (rc = get_plan(e, PK_ENC, c.B, 0, 0, &pe))) return rc;
    const lns_config& cfg = e->cfg;
    const long zper = (long)e->lat_C * e->lat_H * e->lat_W;
    char* base = static_cast<char*>(c.ws);
    Runner r(e, static_cast<hipStream_t>(c.stream));
    begin_run(e, c.ws, c.B);
    if ((rc = arm_sticky(e, r.stream))) return rc;
    ExtT z0 = {c.start, zper};
    if (c.encode) {   // encode once: x -> z0                  (train_stage2_ns2d.py:144)
        ExtT ext[EX_COUNT];
        ext[EX_PARAM] = {c.param, 1};
        ext[EX_IN] = {c.start, (long)cfg.in_channels * cfg.Ly * cfg.Lx};
        ext[EX_OUT] = {base, zper};
        if ((rc = r.run(*pe, ext, base + L.arena_off))) return rc;
        z0.ptr = base;
    }
    // time maps: the horizon's first call clears the state on the caller's stream, which every stream of the loop starts behind
    if (scored && c.maps && c.t0 == 0) HIPCHK(e, hipMemsetAsync(base + L.maps_off, 0, L.maps_bytes, r.stream));
    if (ens && (rc = ensemble_begin(e, c, r.stream))) return rc;   // (ahead of the loop's fork event)
    if ((rc = rollout_loop(e, r, z0, c, L))) return rc;
    // every plane's pair is in place once the decode streams have joined: frame- and sequence-wise ratios, once the
    // horizon is complete (the pairs of the earlier chunks are in the workspace)
    if (scored && c.t0 + c.T == c.T_total)
        HIPCHK(e, launch_metric_finish(reinterpret_cast<float*>(base + L.part_off), c.B, c.T_total, cfg.in_channels, c.spec->eps,
                                       c.frame_out, c.seq_out, r.stream));
    if (scored && c.attrib && c.t0 + c.T == c.T_total) {   // likewise: the three further sum arrays -> the attribution columns
        const lns_eval_attrib& a = c.at;
        if (a.recon_frame || a.recon_seq)
            HIPCHK(e, launch_metric_finish(reinterpret_cast<float*>(base + L.part2_off), c.B, c.T_total, cfg.in_channels, c.spec->eps,
                                           a.recon_frame, a.recon_seq, r.stream));
        if (a.prop_frame || a.prop_seq || a.cross_frame || a.cross_seq)
            HIPCHK(e, launch_attrib_finish(reinterpret_cast<float*>(base + L.ppart_off), c.B, c.T_total, cfg.in_channels,
                                           c.spec->eps, a.prop_frame, a.prop_seq, a.cross_frame, a.cross_seq, r.stream));
        if (a.latent_frame || a.latent_seq)
            HIPCHK(e, launch_metric_finish(reinterpret_cast<float*>(base + L.lpart_off), c.B, c.T_total, 1, c.spec->eps,
                                           a.latent_frame, a.latent_seq, r.stream));
    }
    if (scored && c.maps && c.t0 + c.T == c.T_total) {   // likewise: the state of all chunks -> the seven maps
        TimeMapsArgs tm;
        time_maps_args(e, c, L, &tm);
        HIPCHK(e, launch_time_maps_finish(tm, r.stream));
    }
    if (ens && (rc = ensemble_finish(e, c, L, r.stream))) return rc;
    return r.finish();
}

// The one body of the eight scored entry points (lns_rollout_eval, lns_rollout_latent_eval and their _spectrum / _stats /
// _maps forms): the union of their argument lists.  From x: encode, t0 = 0, T_total = T, no z_last.  The selections come
// loose (the _spectrum and _stats forms; all null / 0 for the plain one) or, for SCORED_MAPS, in `sel`.
enum ScoredForm { SCORED_PLAIN, SCORED_SPECTRUM, SCORED_STATS, SCORED_MAPS, SCORED_ATTRIB, SCORED_FLOW };   // (_ATTRIB: the plain form + `attrib`; _FLOW: a nullable `sel` without maps + `flow`)
static int scored_call(lns_engine* e, ScoredForm form, const float* start, bool encode, const float* param, const float* y_true,
                       int B, int T, int t0, int T_total, const lns_eval_spec* spec, float* frame_out, float* seq_out,
                       const int* keep, int n_keep, float* frames_out, float* z_last, void* ws, size_t ws_bytes, void* stream,
                       const int* spectrum_steps, int n_spec, float* spectra_out, const int* stats_steps, int n_stats,
                       const lns_stats_spec* hspec, float* stats_out, int32_t* hist_out, const lns_eval_select* sel,
                       const lns_eval_attrib* attrib = nullptr, const lns_eval_flow* flow = nullptr) {
    RolloutCall c(start, encode, param, B, T, ws, ws_bytes, stream);
    c.sink = SINK_SCORED;
    c.attrib = form == SCORED_ATTRIB;
    c.at_bad = c.attrib && (!attrib || attrib->size != sizeof(lns_eval_attrib));
    if (c.attrib && !c.at_bad) c.at = *attrib;
    c.y_true = y_true; c.t0 = t0; c.T_total = T_total; c.spec = spec; c.frame_out = frame_out; c.seq_out = seq_out;
    c.keep = keep; c.n_keep = n_keep; c.frames_out = frames_out; c.z_last = z_last;
    c.maps = form == SCORED_MAPS;
    c.sel_bad = c.maps && (!sel || sel->size != sizeof(lns_eval_select));   // (the two selections then count as absent)
    if (c.maps && !c.sel_bad) c.sel = *sel;
    c.flow = form == SCORED_FLOW;
    if (c.flow) {
        c.sel_bad = sel && sel->size != sizeof(lns_eval_select);
        if (sel && !c.sel_bad) c.sel = *sel;
        c.flow_bad = !flow || flow->size != sizeof(lns_eval_flow);
        if (!c.flow_bad) c.fl = *flow;
    }
    if (!c.maps && !c.flow) {
        c.sel.spectrum_steps_host = spectrum_steps; c.sel.n_spec = n_spec; c.sel.spectra_out = spectra_out;
        c.sel.stats_steps_host = stats_steps; c.sel.n_stats = n_stats; c.sel.hspec = hspec; c.sel.stats_out = stats_out;
        c.sel.hist_out = hist_out;
    }
    c.spectra = form == SCORED_SPECTRUM || c.sel.n_spec != 0;
    c.stats = form == SCORED_STATS || c.sel.n_stats != 0;
    return rollout_call(e, c);
}

int lns_rollout(lns_engine* e, const float* x, const float* param, int B, int T, int to_x, float* out,
                float* latents_out, void* ws, size_t ws_bytes, void* stream) {
    RolloutCall c(x, true, param, B, T, ws, ws_bytes, stream);
    c.sink = to_x ? SINK_STEPS : SINK_LATENTS; c.out = out; c.latents_out = latents_out;
    return rollout_call(e, c);
}

int lns_rollout_latent(lns_engine* e, const float* z_in, const float* param, int B, int T, int to_x, float* out,
                       float* z_last, void* ws, size_t ws_bytes, void* stream) {
    RolloutCall c(z_in, false, param, B, T, ws, ws_bytes, stream);
    c.sink = to_x ? SINK_STEPS : SINK_LATENTS; c.out = out; c.z_last = z_last;
    return rollout_call(e, c);
}

// ---- streaming validation rollout (include/lns.h) --------------------------------------------------------------
int lns_rollout_eval(lns_engine* e, const float* x, const float* param, const float* y_true, int B, int T,
                     const lns_eval_spec* spec, float* frame_out, float* seq_out, const int* keep_steps_host, int n_keep,
                     float* frames_out, void* ws, size_t ws_bytes, void* stream) {
    return scored_call(e, SCORED_PLAIN, x, true, param, y_true, B, T, 0, T, spec, frame_out, seq_out, keep_steps_host, n_keep,
                       frames_out, nullptr, ws, ws_bytes, stream, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr);
}

int lns_rollout_latent_eval(lns_engine* e, const float* z_in, const float* param, const float* y_true, int B, int T,
                            int t0, int T_total, const lns_eval_spec* spec, float* frame_out, float* seq_out,
                            const int* keep_steps_host, int n_keep, float* frames_out, float* z_last, void* ws,
                            size_t ws_bytes, void* stream) {
    return scored_call(e, SCORED_PLAIN, z_in, false, param, y_true, B, T, t0, T_total, spec, frame_out, seq_out, keep_steps_host,
                       n_keep, frames_out, z_last, ws, ws_bytes, stream, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr,
                       nullptr);
}

// ---- streaming validation with energy spectra (include/lns.h) ----------------------------------------------------
int lns_rollout_eval_spectrum(lns_engine* e, const float* x, const float* param, const float* y_true, int B, int T,
                              const lns_eval_spec* spec, float* frame_out, float* seq_out, const int* keep_steps_host, int n_keep,
                              float* frames_out, void* ws, size_t ws_bytes, void* stream, const int* spectrum_steps_host,
                              int n_spec, float* spectra_out) {
    return scored_call(e, SCORED_SPECTRUM, x, true, param, y_true, B, T, 0, T, spec, frame_out, seq_out, keep_steps_host, n_keep,
                       frames_out, nullptr, ws, ws_bytes, stream, spectrum_steps_host, n_spec, spectra_out, nullptr, 0, nullptr,
                       nullptr, nullptr, nullptr);
}

int lns_rollout_latent_eval_spectrum(lns_engine* e, const float* z_in, const float* param, const float* y_true, int B, int T,
                                     int t0, int T_total, const lns_eval_spec* spec, float* frame_out, float* seq_out,
                                     const int* keep_steps_host, int n_keep, float* frames_out, float* z_last, void* ws,
                                     size_t ws_bytes, void* stream, const int* spectrum_steps_host, int n_spec,
                                     float* spectra_out) {
    return scored_call(e, SCORED_SPECTRUM, z_in, false, param, y_true, B, T, t0, T_total, spec, frame_out, seq_out,
                       keep_steps_host, n_keep, frames_out, z_last, ws, ws_bytes, stream, spectrum_steps_host, n_spec, spectra_out,
                       nullptr, 0, nullptr, nullptr, nullptr, nullptr);
}

// ---- streaming validation with field statistics (include/lns.h) ---------------------------------------------------
int lns_rollout_eval_stats(lns_engine* e, const float* x, const float* param, const float* y_true, int B, int T,
                           const lns_eval_spec* spec, float* frame_out, float* seq_out, const int* keep_steps_host, int n_keep,
                           float* frames_out, void* ws, size_t ws_bytes, void* stream, const int* spectrum_steps_host, int n_spec,
                           float* spectra_out, const int* stats_steps_host, int n_stats, const lns_stats_spec* hspec,
                           float* stats_out, int32_t* hist_out) {
    return scored_call(e, SCORED_STATS, x, true, param, y_true, B, T, 0, T, spec, frame_out, seq_out, keep_steps_host, n_keep,
                       frames_out, nullptr, ws, ws_bytes, stream, spectrum_steps_host, n_spec, spectra_out, stats_steps_host,
                       n_stats, hspec, stats_out, hist_out, nullptr);
}

int lns_rollout_latent_eval_stats(lns_engine* e, const float* z_in, const float* param, const float* y_true, int B, int T,
                                  int t0, int T_total, const lns_eval_spec* spec, float* frame_out, float* seq_out,
                                  const int* keep_steps_host, int n_keep, float* frames_out, float* z_last, void* ws,
                                  size_t ws_bytes, void* stream, const int* spectrum_steps_host, int n_spec, float* spectra_out,
                                  const int* stats_steps_host, int n_stats, const lns_stats_spec* hspec, float* stats_out,
                                  int32_t* hist_out) {
    return scored_call(e, SCORED_STATS, z_in, false, param, y_true, B, T, t0, T_total, spec, frame_out, seq_out, keep_steps_host,
                       n_keep, frames_out, z_last, ws, ws_bytes, stream, spectrum_steps_host, n_spec, spectra_out,
                       stats_steps_host, n_stats, hspec, stats_out, hist_out, nullptr);
}

// ---- streaming validation with time maps (include/lns.h) ----------------------------------------------------------
int lns_rollout_eval_maps_workspace_bytes(lns_engine* e, int B, size_t* bytes) {
    size_t base = 0;
    if (int rc = workspace_bytes(e, B, SINK_SCORED, &base)) return rc;
    WsLayout L;
    L.total = base;
    add_maps_region(e, B, &L);
    if (bytes) *bytes = L.total;
    return LNS_OK;
}

int lns_rollout_eval_maps(lns_engine* e, const float* x, const float* param, const float* y_true, int B, int T,
                          const lns_eval_spec* spec, float* frame_out, float* seq_out, const int* keep_steps_host, int n_keep,
                          float* frames_out, void* ws, size_t ws_bytes, void* stream, const lns_eval_select* sel) {
    return scored_call(e, SCORED_MAPS, x, true, param, y_true, B, T, 0, T, spec, frame_out, seq_out, keep_steps_host, n_keep,
                       frames_out, nullptr, ws, ws_bytes, stream, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, sel);
}

int lns_rollout_latent_eval_maps(lns_engine* e, const float* z_in, const float* param, const float* y_true, int B, int T,
                                 int t0, int T_total, const lns_eval_spec* spec, float* frame_out, float* seq_out,
                                 const int* keep_steps_host, int n_keep, float* frames_out, float* z_last, void* ws,
                                 size_t ws_bytes, void* stream, const lns_eval_select* sel) {
    return scored_call(e, SCORED_MAPS, z_in, false, param, y_true, B, T, t0, T_total, spec, frame_out, seq_out, keep_steps_host,
                       n_keep, frames_out, z_last, ws, ws_bytes, stream, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr,
                       sel);
}

// ---- streaming validation with error attribution (include/lns.h) --------------------------------------------------
int lns_rollout_eval_attrib_workspace_bytes(lns_engine* e, int B, size_t* bytes) {
    if (int rc = workspace_bytes(e, B, SINK_SCORED, nullptr)) return rc;
    DeviceGuard dg(e);
    WsLayout L;
    if (int rc = ws_layout(e, B, SINK_SCORED, &L)) return rc;
    add_attrib_region(e, B, &L);
    if (bytes) *bytes = L.total;
    return LNS_OK;
}

int lns_rollout_eval_attrib(lns_engine* e, const float* x, const float* param, const float* y_true, int B, int T,
                            const lns_eval_spec* spec, float* frame_out, float* seq_out, const int* keep_steps_host, int n_keep,
                            float* frames_out, const lns_eval_attrib* attrib, void* ws, size_t ws_bytes, void* stream) {
    return scored_call(e, SCORED_ATTRIB, x, true, param, y_true, B, T, 0, T, spec, frame_out, seq_out, keep_steps_host, n_keep,
                       frames_out, nullptr, ws, ws_bytes, stream, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr,
                       attrib);
}

int lns_rollout_latent_eval_attrib(lns_engine* e, const float* z_in, const float* param, const float* y_true, int B, int T,
                                   int t0, int T_total, const lns_eval_spec* spec, float* frame_out, float* seq_out,
                                   const int* keep_steps_host, int n_keep, float* frames_out, float* z_last,
                                   const lns_eval_attrib* attrib, void* ws, size_t ws_bytes, void* stream) {
    return scored_call(e, SCORED_ATTRIB, z_in, false, param, y_true, B, T, t0, T_total, spec, frame_out, seq_out, keep_steps_host,
                       n_keep, frames_out, z_last, ws, ws_bytes, stream, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr,
                       nullptr, attrib);
}

// ---- streaming validation with flow diagnostics (include/lns.h) ---------------------------------------------------
int lns_rollout_eval_flow(lns_engine* e, const float* x, const float* param, const float* y_true, int B, int T,
                          const lns_eval_spec* spec, float* frame_out, float* seq_out, const int* keep_steps_host, int n_keep,
                          float* frames_out, void* ws, size_t ws_bytes, void* stream, const lns_eval_select* sel,
                          const lns_eval_flow* flow) {
    return scored_call(e, SCORED_FLOW, x, true, param, y_true, B, T, 0, T, spec, frame_out, seq_out, keep_steps_host, n_keep,
                       frames_out, nullptr, ws, ws_bytes, stream, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, sel,
                       nullptr, flow);
}

int lns_rollout_latent_eval_flow(lns_engine* e, const float* z_in, const float* param, const float* y_true, int B, int T,
                                 int t0, int T_total, const lns_eval_spec* spec, float* frame_out, float* seq_out,
                                 const int* keep_steps_host, int n_keep, float* frames_out, float* z_last, void* ws,
                                 size_t ws_bytes, void* stream, const lns_eval_select* sel, const lns_eval_flow* flow) {
    return scored_call(e, SCORED_FLOW, z_in, false, param, y_true, B, T, t0, T_total, spec, frame_out, seq_out, keep_steps_host,
                       n_keep, frames_out, z_last, ws, ws_bytes, stream, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr,
                       sel, nullptr, flow);
}

// ---- stage-1 validation (include/lns.h) ---------------------------------------------------------------------------
// the evaluation layout for an engine that may lack the propagator (ws_layout sizes a missing propagator's arena as 0)
int lns_autoencode_eval_workspace_bytes(lns_engine* e, int B, size_t* bytes) {
    if (!e) return LNS_EINVAL;
    if (B <= 0) return einval(e, "B must be positive");
    if (int brc = check_batch(e, B)) return brc;
    if (e->enc.empty()) { e->err = "autoencode_eval needs an autoencoder"; return LNS_ESTATE; }
    DeviceGuard dg(e);
    WsLayout L;
    if (int rc = ws_layout(e, B, SINK_SCORED, &L)) return rc;
    if (bytes) *bytes = L.total;
    return LNS_OK;
}

// x[:, t] -> z -> the frame buffer -> the metric's pair of plane (b, t, c) against x[:, t] itself, step by step on the
// caller's stream in the first decode arena (stream order is the whole hazard argument); then the metric's finish kernel
int lns_autoencode_eval(lns_engine* e, const float* x, const float* param, int B, int T, const lns_eval_spec* spec,
                        float* frame_out, float* seq_out, float* z_out, void* ws, size_t ws_bytes, void* stream) {
    if (!e) return LNS_EINVAL;
    RolloutCall c(x, true, param, B, T, ws, ws_bytes, stream);
    c.sink = SINK_SCORED; c.ae_only = true;
    c.y_true = x; c.t0 = 0; c.T_total = T; c.spec = spec; c.frame_out = frame_out; c.seq_out = seq_out;
    int rc;
    if ((rc = rollout_refusal(e, c))) return rc;
    DeviceGuard dg(e);
    WsLayout L;
    if ((rc = ws_layout(e, B, SINK_SCORED, &L)) || (rc = check_ws(e, L, "evaluation ", ws, ws_bytes))) return rc;
    Plan *pe, *pd;
    if ((rc = get_plan(e, PK_ENC, B, 0, 0, &pe)) || (rc = get_plan(e, PK_DEC, B, 0, 0, &pd))) return rc;
    const long zper = (long)e->lat_C * e->lat_H * e->lat_W;
    const long xper = (long)e->cfg.in_channels * e->cfg.Ly * e->cfg.Lx;
    char* base = static_cast<char*>(ws);
    Runner r(e, static_cast<hipStream_t>(stream));
    begin_run(e, ws, B);
    if ((rc = arm_sticky(e, r.stream))) return rc;
    MetricGroupArgs m;
    metric_args(e, c, L, &m);
    float* fb = reinterpret_cast<float*>(base + L.fbuf_off);
    m.frames = fb; m.kk = 1;
    ExtT ext[EX_COUNT];
    ext[EX_PARAM] = {param, 1};
    for (int t = 0; t < T; ++t) {
        // the latent goes straight to its slot of z_out where the caller wants it, else to the layout's z0 buffer
        const ExtT z = z_out ? ExtT{z_out + (long)t * zper, (long)T * zper} : ExtT{base, zper};
        ext[EX_IN] = {x + (long)t * xper, (long)T * xper};
        ext[EX_OUT] = z;
        if ((rc = r.run(*pe, ext, base + L.arena_off))) return rc;
        ext[EX_IN] = z;
        ext[EX_OUT] = {fb, xper};
        if ((rc = r.run(*pd, ext, base + L.arena_off))) return rc;
        m.y_t = t; m.p_t = t;
        HIPCHK(e, launch_metric_group(m, r.stream));
    }
    HIPCHK(e, launch_metric_finish(reinterpret_cast<float*>(base + L.part_off), B, T, e->cfg.in_channels, spec->eps, frame_out, seq_out,
                                   r.stream));
    return r.finish();
}

// ---- selected-step rollout (include/lns.h) ----------------------------------------------------------------------
int lns_rollout_select(lns_engine* e, const float* x, const float* param, int B, int T, const int* keep_steps_host,
                       int n_keep, float* out, float* latents_out, void* ws, size_t ws_bytes, void* stream) {
    RolloutCall c(x, true, param, B, T, ws, ws_bytes, stream);
    c.sink = SINK_KEPT; c.keep = keep_steps_host; c.n_keep = n_keep; c.out = out; c.latents_out = latents_out;
    return rollout_call(e, c);
}

int lns_rollout_latent_select(lns_engine* e, const float* z_in, const float* param, int B, int T,
                              const int* keep_steps_host, int n_keep, float* out, float* z_last, void* ws, size_t ws_bytes,
                              void* stream) {
    RolloutCall c(z_in, false, param, B, T, ws, ws_bytes, stream);
    c.sink = SINK_KEPT; c.keep = keep_steps_host; c.n_keep = n_keep; c.out = out; c.z_last = z_last;
    return rollout_call(e, c);
}

// ---- ensemble rollout (include/lns.h) --------------------------------------------------------------------------
// What the six ensemble entry points share of their RolloutCall; each adds the fields of its form
static RolloutCall ensemble_call(EnsForm form, const float* z_in, const float* param, int B, int M, int T, const int* keep_steps_host,
                                 int n_keep, float* mean_out, float* var_out, float* z_last, void* ws, size_t ws_bytes, void* stream) {
    RolloutCall c(z_in, false, param, ensemble_batch(B, M), T, ws, ws_bytes, stream);
    c.sink = SINK_ENSEMBLE; c.ens_form = form; c.traj = B; c.M = M; c.keep = keep_steps_host; c.n_keep = n_keep;
    c.out = mean_out; c.var_out = var_out; c.z_last = z_last;
    return c;
}

int lns_rollout_latent_ensemble(lns_engine* e, const float* z_in, const float* param, int B, int M, int T,
                                const int* keep_steps_host, int n_keep, float* mean_out, float* var_out, float* z_last,
                                void* ws, size_t ws_bytes, void* stream) {
    return rollout_call(e, ensemble_call(ENS_STATS, z_in, param, B, M, T, keep_steps_host, n_keep, mean_out, var_out, z_last, ws, ws_bytes, stream));
}

// ---- ensemble validation (include/lns.h) ------------------------------------------------------------------------
int lns_rollout_latent_ensemble_eval(lns_engine* e, const float* z_in, const float* param, const float* y_true, int B, int M, int T,
                                     const int* keep_steps_host, int n_keep, const lns_eval_spec* spec, float* scores_out,
                                     float* seq_out, int32_t* rank_out, float* mean_out, float* var_out, float* z_last,
                                     void* ws, size_t ws_bytes, void* stream) {
    RolloutCall c = ensemble_call(ENS_SCORED, z_in, param, B, M, T, keep_steps_host, n_keep, mean_out, var_out, z_last, ws, ws_bytes, stream);
    c.y_true = y_true; c.spec = spec; c.scores_out = scores_out; c.seq_out = seq_out; c.rank_out = rank_out;
    return rollout_call(e, c);
}

// ---- ensemble quantiles (include/lns.h) -------------------------------------------------------------------------
int lns_rollout_latent_ensemble_quantiles(lns_engine* e, const float* z_in, const float* param, int B, int M, int T,
                                          const int* keep_steps_host, int n_keep, const lns_ensemble_quantile_spec* qspec,
                                          const lns_eval_spec* norm, float* quant_out, float* prob_out, float* mean_out,
                                          float* var_out, float* z_last, void* ws, size_t ws_bytes, void* stream) {
    RolloutCall c = ensemble_call(ENS_QUANT, z_in, param, B, M, T, keep_steps_host, n_keep, mean_out, var_out, z_last, ws, ws_bytes, stream);
    c.qspec = qspec; c.spec = norm; c.quant_out = quant_out; c.prob_out = prob_out;
    return rollout_call(e, c);
}

// ---- ensemble exceedance tables (include/lns.h) -----------------------------------------------------------------
int lns_rollout_latent_ensemble_exceed(lns_engine* e, const float* z_in, const float* param, const float* y_true, int B, int M, int T,
                                       const int* keep_steps_host, int n_keep, const lns_ensemble_exceed_spec* xspec,
                                       const lns_eval_spec* norm, int32_t* table_out, float* mean_out, float* var_out,
                                       float* z_last, void* ws, size_t ws_bytes, void* stream) {
    RolloutCall c = ensemble_call(ENS_EXCEED, z_in, param, B, M, T, keep_steps_host, n_keep, mean_out, var_out, z_last, ws, ws_bytes, stream);
    c.xspec = xspec; c.spec = norm; c.y_true = y_true; c.table_out = table_out;
    return rollout_call(e, c);
}

// ---- ensemble transform Kalman filter, global and localised (include/lns.h) -------------------------------------
// the size query of either analysis form: the ensemble layout and the form's region behind it
static int analysis_workspace_bytes(lns_engine* e, EnsForm form, int B, int M, int n_keep, size_t* bytes) {
    if (!e) return LNS_EINVAL;
    if (B <= 0) return einval(e, "B must be positive");
    if (M <= 0) return einval(e, "M must be positive");
    if (int mrc = analysis_members_refusal(e, M)) return mrc;
    if (n_keep < 1) return einval(e, "n_keep must be at least 1");
    if (form == ENS_ANALYSIS_LOCAL && (long)e->lat_H * e->lat_W > LNS_LETKF_MAX_DOMAINS)
        return einval(e, "local ensemble analysis needs a latent grid of at most 4096 pixels");
    size_t base = 0;
    if (int rc = workspace_bytes(e, ensemble_batch(B, M), SINK_ENSEMBLE, &base)) return rc;
    if (bytes) *bytes = round_up_sz(base, 256) + analysis_region(e, form, B, M, n_keep).bytes;
    return LNS_OK;
}
int lns_rollout_ensemble_analysis_workspace_bytes(lns_engine* e, int B, int M, int n_keep, size_t* bytes) { return analysis_workspace_bytes(e, ENS_ANALYSIS, B, M, n_keep, bytes); }
int lns_rollout_ensemble_analysis_local_workspace_bytes(lns_engine* e, int B, int M, int n_keep, size_t* bytes) { return analysis_workspace_bytes(e, ENS_ANALYSIS_LOCAL, B, M, n_keep, bytes); }

// what the two analysis entry points add to ensemble_call's RolloutCall alike: the observations and the global filter's outputs
static void analysis_fields(RolloutCall* c, const float* y_obs, const float* rinv, int64_t rinv_bs, int64_t rinv_ss, const lns_eval_spec* norm,
                            double rho, float* z_analysis, float* param_analysis, double* X_out, double* wbar_out, double* lam_out,
                            double* stat_out, int32_t* status_out) {
    c->y_true = y_obs; c->rinv = rinv; c->rinv_bs = rinv_bs; c->rinv_ss = rinv_ss; c->spec = norm; c->rho = rho;
    c->z_analysis = z_analysis; c->param_analysis = param_analysis; c->X_out = X_out; c->wbar_out = wbar_out; c->lam_out = lam_out;
    c->stat_out = stat_out; c->status_out = status_out;
    c->z_last = c->z_last ? c->z_last : z_analysis;  // the forecast latents of step T - 1: the update reads them (in place without z_last)
}

int lns_rollout_latent_ensemble_analysis(lns_engine* e, const float* z_in, const float* param, const float* y_obs, const float* rinv,
                                         int64_t rinv_bs, int64_t rinv_ss, int B, int M, int T, const int* keep_steps_host, int n_keep,
                                         const lns_eval_spec* norm, double rho, float* z_analysis, float* param_analysis, double* X_out,
                                         double* wbar_out, double* lam_out, double* stat_out, int32_t* status_out, float* mean_out,
                                         float* var_out, float* z_last, void* ws, size_t ws_bytes, void* stream) {
    RolloutCall c = ensemble_call(ENS_ANALYSIS, z_in, param, B, M, T, keep_steps_host, n_keep, mean_out, var_out, z_last, ws, ws_bytes, stream);
    analysis_fields(&c, y_obs, rinv, rinv_bs, rinv_ss, norm, rho, z_analysis, param_analysis, X_out, wbar_out, lam_out, stat_out, status_out);
    return rollout_call(e, c);
}

int lns_rollout_latent_ensemble_analysis_local(lns_engine* e, const float* z_in, const float* param, const float* y_obs, const float* rinv,
                                               int64_t rinv_bs, int64_t rinv_ss, int B, int M, int T, const int* keep_steps_host,
                                               int n_keep, const lns_eval_spec* norm, double rho, double loc_radius, int bc_y, int bc_x,
                                               float* z_analysis, double* X_local, double* wbar_local, double* lam_local,
                                               int32_t* status_local, float* param_analysis, double* X_out, double* wbar_out,
                                               double* lam_out, double* stat_out, int32_t* status_out, float* mean_out, float* var_out,
                                               float* z_last, void* ws, size_t ws_bytes, void* stream) {
    RolloutCall c = ensemble_call(ENS_ANALYSIS_LOCAL, z_in, param, B, M, T, keep_steps_host, n_keep, mean_out, var_out, z_last, ws, ws_bytes, stream);
    analysis_fields(&c, y_obs, rinv, rinv_bs, rinv_ss, norm, rho, z_analysis, param_analysis, X_out, wbar_out, lam_out, stat_out, status_out);
    c.loc_radius = loc_radius; c.bc_y = bc_y; c.bc_x = bc_x;
    c.X_loc_out = X_local; c.wbar_loc_out = wbar_local; c.lam_loc_out = lam_local; c.status_loc_out = status_local;
    return rollout_call(e, c);
}

int lns_check_finite(lns_engine* e, int B, void* ws, size_t ws_bytes, void* stream) {
    if (!e || B <= 0 || !ws) return LNS_EINVAL;
    // The amax vectors live in the CALLER's workspace: they are read through the `ws` handed in here, which must be
    // the workspace (and batch) of the last run; plans are looked up again by key, so a call after
    // lns_finalize_weights / a dropped plan reports LNS_ESTATE instead of touching freed memory.
    if (e->ran.empty() || e->ran_ws != ws || e->ran_B != B) {
        e->err = e->ran.empty() ? "lns_check_finite: no run to check (call it right after encode / decode / propagate / rollout)"
                                : "lns_check_finite: the last run used a different workspace or batch";
        return LNS_ESTATE;
    }
    DeviceGuard dg(e);
    HIPCHK(e, hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    std::vector<unsigned> host;
    for (const auto& rr : e->ran) {                        // in the order the last call first ran them
        auto& m = rr.kind == PK_ENC ? e->enc_plans : (rr.kind == PK_DEC ? e->dec_plans : e->prop_plans);
        auto it = m.find(rr.key);
        if (it == m.end()) { e->err = "lns_check_finite: the plan of the last run was dropped"; return LNS_ESTATE; }
        const Plan& p = it->second;
        if (!p.amax_bytes) continue;
        if (rr.arena_off + p.amax_off + p.amax_bytes > ws_bytes) {
            e->err = fmt("lns_check_finite: workspace of %zu bytes does not hold the last run's arena", ws_bytes);
            return LNS_ENOMEM;
        }
        host.resize(p.amax_bytes / 4);
        HIPCHK(e, hipMemcpy(host.data(), static_cast<const char*>(ws) + rr.arena_off + p.amax_off, p.amax_bytes, hipMemcpyDeviceToHost));
        const char* what = rr.kind == PK_ENC ? "encoder" : (rr.kind == PK_DEC ? "decoder" : "propagator");
        const size_t per = (size_t)p.B * LNS_AMAX_SUB;
        for (size_t i = 0; i < p.amax_names.size(); ++i)
            for (size_t bk = 0; bk < per; ++bk)
                if (((host[i * per + bk] >> 23) & 0xffu) == 0xffu) {
                    const int s = (int)(bk / LNS_AMAX_SUB);   // launch sample; step-batched decodes: s = step-in-group * B + trajectory
                    e->err = fmt("non-finite values in the output of %s (%s, sample %d)", p.amax_names[i].c_str(), what, s % B);
                    return LNS_ENONFINITE;
                }
    }
    if (e->sticky_armed && e->d_sticky) {                  // runs whose amax region has been reused since (earlier steps / groups)
        unsigned st[4] = {0, 0, 0, 0};
        HIPCHK(e, hipMemcpy(st, e->d_sticky, 16, hipMemcpyDeviceToHost));
        for (int k = 0; k < 3; ++k)
            if (st[k]) {
                e->err = fmt("non-finite values in an earlier %s run of the last call (its amax record has been reused since)",
                             k == PK_ENC ? "encoder" : (k == PK_DEC ? "decoder" : "propagator"));
                return LNS_ENONFINITE;
            }
    }
    return LNS_OK;
}

// ---- diagnostics -------------------------------------------------------------
int lns_trace_enable(lns_engine* e, int on) { if (!e) return LNS_EINVAL; e->trace_on = on != 0; e->trace.clear(); return LNS_OK; }
int lns_trace_count(const lns_engine* e) { return e ? (int)e->trace.size() : LNS_EINVAL; }
int lns_trace_info(const lns_engine* e, int i, char* name, int cap, int64_t* shape) {
    if (!e || i < 0 || i >= (int)e->trace.size()) return LNS_EINVAL;
    const TraceRec& r = e->trace[i];
    if (name && cap > 0) { strncpy(name, r.name.c_str(), cap - 1); name[cap - 1] = 0; }
    if (shape) { shape[0] = r.B; shape[1] = r.C; shape[2] = r.H; shape[3] = r.W; }
    return LNS_OK;
}
int lns_trace_copy(const lns_engine* e, int i, float* host_out) {
    if (!e || i < 0 || i >= (int)e->trace.size() || !host_out) return LNS_EINVAL;
    memcpy(host_out, e->trace[i].data.data(), e->trace[i].data.size() * 4);
    return LNS_OK;
}
int lns_timing_enable(lns_engine* e, int on) { if (!e) return LNS_EINVAL; e->timing_on = on != 0; e->timing.clear(); return LNS_OK; }
int lns_timing_count(const lns_engine* e) { return e ? (int)e->timing.size() : LNS_EINVAL; }
int lns_timing_info(const lns_engine* e, int i, char* name, int cap, double* ms, int64_t* launches, double* flops,
                    double* bytes) {
    if (!e || i < 0 || i >= (int)e->timing.size()) return LNS_EINVAL;
    const TimeRec& t = e->timing[i];
    if (name && cap > 0) { strncpy(name, t.name.c_str(), cap - 1); name[cap - 1] = 0; }
    if (ms) *ms = t.ms;
    if (launches) *launches = t.launches;
    if (flops) *flops = t.flops;
    if (bytes) *bytes = t.bytes;
    return LNS_OK;
}

int lns_timing_mfma_flops(const lns_engine* e, int i, double* mfma_flops) {
    if (e && i == -1 && mfma_flops) { *mfma_flops = e->timing_overhead_ms * 1e3; return LNS_OK; }     // index -1: see include/lns.h
    if (!e || i < 0 || i >= (int)e->timing.size() || !mfma_flops) return LNS_EINVAL;
    *mfma_flops = e->timing[i].mfma_flops;
    return LNS_OK;
}

// ---- kernel-level entry points (tests) ------------------------------------------
int lns_build_has(const char* feature) {
    if (!feature) return -1;
    if (!strcmp(feature, "experimental")) return build_has_experimental() ? 1 : 0;
    if (!strcmp(feature, "train_wgrad_split")) return 1;
    if (!strcmp(feature, "train_clip")) return 1;
    if (!strcmp(feature, "train_ops")) return 1;
    if (!strcmp(feature, "latent_fit")) return 1;
    if (!strcmp(feature, "rollout_tangent")) return 1;
    if (!strcmp(feature, "fit_gauss_newton")) return 1;
    if (!strcmp(feature, "rollout_select")) return 1;
    if (!strcmp(feature, "rollout_ensemble")) return 1;
    if (!strcmp(feature, "ensemble_score")) return 1;
    if (!strcmp(feature, "ensemble_quantiles")) return 1;
    if (!strcmp(feature, "ensemble_exceed")) return 1;
    if (!strcmp(feature, "ensemble_etkf")) return 1;
    if (!strcmp(feature, "ensemble_letkf")) return 1;
    if (!strcmp(feature, "eval_spectrum")) return 1;
    if (!strcmp(feature, "spectrum_basis")) return 1;
    if (!strcmp(feature, "eval_stats")) return 1;
    if (!strcmp(feature, "eval_maps")) return 1;
    if (!strcmp(feature, "eval_attrib")) return 1;
    if (!strcmp(feature, "eval_flow")) return 1;
    if (!strcmp(feature, "op_conv_gn")) return 1;
    if (!strcmp(feature, "op_fa_fused")) return 1;
    if (!strcmp(feature, "op_fa_axis")) return 1;
#ifdef LNS_DIAG
    if (!strcmp(feature, "diag")) return 1;
#else
    if (!strcmp(feature, "diag")) return 0;
#endif
    return -1;
}

#include "lns_ops.inc"

}  // extern "C"

#include "lns_train.inc"
#include "lns_tangent.inc"
#include "lns_fit_gn.inc"

// The kernel-form switches of the library: every LNS_* environment variable csrc/ reads, declared once.  A switch is a field of
// Knobs and a row of kKnobRows; the parser loops over the rows, so a switch cannot exist without its row, and README's
// environment table is a copy of the rows' text (tests/test_knobs_cpu.py holds the two together).
//   knobs()            the process switches: read from the environment at the first call, never again.  The planner and the
//                      launcher of one launch therefore see the same values, and the form rules of lns_kernels.h
//                      (attn_is_f16, fa_sandwich_form, ...) are asked by both.
//   option_defaults()  the nine variables that are defaults of per-engine options (lns_set_option): parsed at every call, that
//                      is at every lns_create -- a process may set one between two engines.
// A variable that is unset parses its row's default text, so a default stands in one place.  Flags are "set or not" (any value,
// the empty one included, switches them on); counts go through atol.
// Host only, no HIP: tests/native/knobs_check.cpp and conv_launch_check.cpp compile it with the host compiler.
// Not in the table: the reads of diagnostic builds (LNS_TS_*, LNS_SKIP_OPS under their #if, LNS_STRESS_* in the pair-stress op).
#pragma once
#include <cstdlib>
#include <cstring>

namespace lns {

enum Conv3Split { CONV3_SPLIT_F16X2 = 0, CONV3_SPLIT_BF16X3 = 1 };

struct Knobs {
    // GroupNorm from conv-epilogue tile statistics
    bool gn_no_fuse, gn_no_fold, gn_no_ragged, gn_no_ragged_tiles;
    long gn_fuse_min_hw, gn_fold_tiles;
    // convolutions
    bool conv_fp32_mfma, conv1_fp32_mfma, conv1_no_thin, conv1_no_stationary, conv_use_128, conv_kcl4;
    long conv1s_min_blocks, conv_min_blocks, convb32_below, convf32_below, conv_w8_below;
    Conv3Split conv3_split;
    bool no_fuse_1x1, no_gelu_prologue, no_arith_maps;
    // upsampling 3x3 convolutions
    bool no_up2_phases, up2_quad, up2_resident;
    // FABlock2D, attention
    bool fa_sandwich_fp32, fa_sandwich_bf16x3, fa_sandwich_3wave, fa_fused_no_small, fa_no_fuse_to_out, fa_no_merge, fa_no_reverse,
         fa_reducer_scalar, attn_fp32;
    long fa_ppb;
    // batch-parallel weight gradient
    long wgrad_target_blocks, wgrad_max_slices;
    // diagnosis
    bool debug_sync, timing_by_name;
};

// what lns_create copies into the engine's opt_* fields (clamps and option names: lns_create, lns_set_option)
struct OptionDefaults {
    long decode_group, decode_streams, no_overlap, prop_priority, fa_chunk_mb, fa_fused, fa_fused_gpb, no_fold_linear, up2_dual;
};

enum KnobKind { KNOB_FLAG, KNOB_COUNT, KNOB_CONV3_SPLIT, KNOB_OPTION_FLAG, KNOB_OPTION_COUNT };
inline const char* knob_kind_name(KnobKind k) {
    switch (k) {
        case KNOB_FLAG: return "flag";
        case KNOB_COUNT: return "count";
        case KNOB_CONV3_SPLIT: return "name";
        case KNOB_OPTION_FLAG: return "option default (flag)";
        default: return "option default (count)";
    }
}

struct KnobRow {
    const char* env; KnobKind kind; const char* dflt; const char* doc;
    bool Knobs::*flag; long Knobs::*count; long OptionDefaults::*option;     // the one that goes with `kind`
};
constexpr KnobRow knob_flag(const char* env, bool Knobs::*f, const char* doc) { return {env, KNOB_FLAG, "off", doc, f, nullptr, nullptr}; }
constexpr KnobRow knob_count(const char* env, long Knobs::*f, const char* dflt, const char* doc) {
    return {env, KNOB_COUNT, dflt, doc, nullptr, f, nullptr};
}
constexpr KnobRow option_flag(const char* env, long OptionDefaults::*f, const char* doc) {
    return {env, KNOB_OPTION_FLAG, "off", doc, nullptr, nullptr, f};
}
constexpr KnobRow option_count(const char* env, long OptionDefaults::*f, const char* dflt, const char* doc) {
    return {env, KNOB_OPTION_COUNT, dflt, doc, nullptr, nullptr, f};
}

constexpr KnobRow kKnobRows[] = {
    knob_flag("LNS_GN_NO_FUSE", &Knobs::gn_no_fuse, "no GroupNorm statistics in the conv epilogue: a statistics launch per GroupNorm"),
    knob_flag("LNS_GN_NO_FOLD", &Knobs::gn_no_fold, "tile partials are merged by a finalize launch, never in the consumer conv's prologue"),
    knob_count("LNS_GN_FUSE_MIN_HW", &Knobs::gn_fuse_min_hw, "256", "smallest plane (pixels) whose GroupNorm takes the tile statistics; default 1024 under LNS_GN_NO_FOLD"),
    knob_flag("LNS_GN_NO_RAGGED", &Knobs::gn_no_ragged, "no tile statistics for planes the 128-pixel tiles do not cover exactly"),
    knob_flag("LNS_GN_NO_RAGGED_TILES", &Knobs::gn_no_ragged_tiles, "ragged planes of one tile only, not of several unequal tiles"),
    knob_count("LNS_GN_FOLD_TILES", &Knobs::gn_fold_tiles, "2", "most tile partials per channel a consumer conv merges in its prologue"),
    knob_flag("LNS_CONV_FP32_MFMA", &Knobs::conv_fp32_mfma, "no split-operand conv kernels (bench strict_fp32 arm); also no phase form, GELU prologue, fused FABlock"),
    knob_flag("LNS_CONV1_FP32_MFMA", &Knobs::conv1_fp32_mfma, "1x1 convs on fp32 MFMA (bench strict_fp32 arm); also no fused FABlock"),
    knob_flag("LNS_CONV1_NO_THIN", &Knobs::conv1_no_thin, "no streaming VALU kernel for 1x1 convs of <= 4 output channels"),
    knob_flag("LNS_CONV1_NO_STATIONARY", &Knobs::conv1_no_stationary, "no input-stationary form of the split 1x1 conv"),
    knob_count("LNS_CONV1S_MIN_BLOCKS", &Knobs::conv1s_min_blocks, "512", "block-count target of the input-stationary 1x1 form (cout tiles per block)"),
    knob_flag("LNS_CONV_USE_128", &Knobs::conv_use_128, "fp32 MFMA convs of > 64 couts try the 128-cout tiles first (tile choice only)"),
    knob_count("LNS_CONV_MIN_BLOCKS", &Knobs::conv_min_blocks, "128", "fp32 MFMA convs: take the next smaller tile below this many blocks"),
    knob_count("LNS_CONVB32_BELOW", &Knobs::convb32_below, "0", "bf16x3 3x3: 32-cout tiles below this many blocks (same bits)"),
    knob_count("LNS_CONVF32_BELOW", &Knobs::convf32_below, "100", "f16x2 3x3: 32-cout tiles below this many blocks (same bits)"),
    knob_flag("LNS_CONV_KCL4", &Knobs::conv_kcl4, "3x3 convs on fp32 MFMA prefer LDS stages of 4 input channels to stages of 8"),
    knob_count("LNS_CONV_W8_BELOW", &Knobs::conv_w8_below, "0", "f16x2 3x3: the eight-wave kernel below this many blocks (same bits)"),
    {"LNS_CONV3_SPLIT", KNOB_CONV3_SPLIT, "f16x2", "operand split of the 3x3 convs: bf16x3 selects the three-term bf16 kernels, any other value is f16x2",
     nullptr, nullptr, nullptr},
    knob_flag("LNS_NO_FUSE_1X1", &Knobs::no_fuse_1x1, "a following 64 -> 64 1x1 conv is its own launch, not the first conv's epilogue"),
    knob_flag("LNS_NO_GELU_PROLOGUE", &Knobs::no_gelu_prologue, "GroupNorm -> GELU -> conv materialises the activation (conditional block)"),
    knob_flag("LNS_NO_ARITH_MAPS", &Knobs::no_arith_maps, "split 3x3 kernels read their source maps from tables everywhere"),
    knob_flag("LNS_NO_UP2_PHASES", &Knobs::no_up2_phases, "upsampling 3x3 convs in the nine-tap gather form, no phase-decomposed weights"),
    knob_flag("LNS_UP2_QUAD", &Knobs::up2_quad, "quad-phase form of the upsampling conv (experimental builds); inert under LNS_UP2_RESIDENT"),
    knob_flag("LNS_UP2_RESIDENT", &Knobs::up2_resident, "resident-patch form of the upsampling conv where it fits"),
    knob_flag("LNS_FA_SANDWICH_FP32", &Knobs::fa_sandwich_fp32, "FABlock sandwich on fp32 MFMA (bench strict_fp32 arm); also no fused FABlock"),
    knob_flag("LNS_FA_SANDWICH_BF16X3", &Knobs::fa_sandwich_bf16x3, "the three-term bf16 sandwich instead of f16x2; also no fused FABlock"),
    knob_flag("LNS_FA_SANDWICH_3WAVE", &Knobs::fa_sandwich_3wave, "three-wave bf16x3 sandwich where four waves' LDS image does not fit (default there: fp32 MFMA)"),
    knob_count("LNS_FA_PPB", &Knobs::fa_ppb, "64", "most planes per block of the f16x2 and bf16x3 sandwich kernels"),
    knob_flag("LNS_FA_FUSED_NO_SMALL", &Knobs::fa_fused_no_small, "fused FABlock kernel for 64-row planes only"),
    knob_flag("LNS_FA_NO_FUSE_TO_OUT", &Knobs::fa_no_fuse_to_out, "FABlock to_out.1 and to_out.3 as two launches"),
    knob_flag("LNS_FA_NO_MERGE", &Knobs::fa_no_merge, "FABlock reducers and low-rank kernels: one launch per axis"),
    knob_flag("LNS_FA_NO_REVERSE", &Knobs::fa_no_reverse, "sandwich kernels walk the samples in launch order (scheduling only)"),
    knob_flag("LNS_FA_REDUCER_SCALAR", &Knobs::fa_reducer_scalar, "scalar form of the FABlock PoolingReducer where the MFMA form would run"),
    knob_flag("LNS_ATTN_FP32", &Knobs::attn_fp32, "attention on fp32 MFMA (bench strict_fp32 arm)"),
    knob_count("LNS_WGRAD_TARGET_BLOCKS", &Knobs::wgrad_target_blocks, "512", "batch-parallel weight gradient: blocks per launch aimed at; values below 1 give the default"),
    knob_count("LNS_WGRAD_MAX_SLICES", &Knobs::wgrad_max_slices, "128", "batch-parallel weight gradient: most partial sums per element; values below 1 give the default"),
    knob_flag("LNS_DEBUG_SYNC", &Knobs::debug_sync, "name every launch on stderr and wait for it (diagnosis of a device fault)"),
    knob_flag("LNS_TIMING_BY_NAME", &Knobs::timing_by_name, "timing records per layer name instead of per kernel class"),
    option_count("LNS_DECODE_GROUP", &OptionDefaults::decode_group, "1", "default of option decode_group: steps decoded per launch set, 0 = automatic"),
    option_count("LNS_DECODE_STREAMS", &OptionDefaults::decode_streams, "3", "default of option decode_streams"),
    option_flag("LNS_NO_OVERLAP", &OptionDefaults::no_overlap, "default of option overlap = 0: everything on the caller's stream"),
    option_flag("LNS_PROP_PRIORITY", &OptionDefaults::prop_priority, "default of option prop_priority = 1: the propagator's stream at the highest priority"),
    option_count("LNS_FA_CHUNK_MB", &OptionDefaults::fa_chunk_mb, "0", "default of option fa_chunk_mb: FABlock chain re-issued per group of samples of this size, 0 = off"),
    option_count("LNS_FA_FUSED", &OptionDefaults::fa_fused, "2", "default of option fa_fused: fused FABlock kernel double-buffered 2, single-buffered 1, generic 3, off 0"),
    option_count("LNS_FA_FUSED_GPB", &OptionDefaults::fa_fused_gpb, "0", "default of option fa_fused_gpb: plane groups per block, 0 = automatic"),
    option_flag("LNS_NO_FOLD_LINEAR", &OptionDefaults::no_fold_linear, "default of option fold_linear = 0: adjacent linear convs keep their own weights"),
    option_count("LNS_UP2_DUAL", &OptionDefaults::up2_dual, "1", "default of option up2_dual: dual-phase upsampling conv where it fits, 0 = one block per output phase"),
};
constexpr int kKnobRowCount = (int)(sizeof kKnobRows / sizeof kKnobRows[0]);

// one pass over the rows: process rows into *k, option rows into *o (either may be null)
inline void parse_knob_rows(Knobs* k, OptionDefaults* o) {
    for (const KnobRow& r : kKnobRows) {
        const char* v = getenv(r.env);
        switch (r.kind) {
            case KNOB_FLAG: if (k) k->*r.flag = v != nullptr; break;
            case KNOB_COUNT: if (k) k->*r.count = atol(v ? v : r.dflt); break;
            case KNOB_CONV3_SPLIT: if (k) k->conv3_split = strcmp(v ? v : r.dflt, "bf16x3") == 0 ? CONV3_SPLIT_BF16X3 : CONV3_SPLIT_F16X2; break;
            case KNOB_OPTION_FLAG: if (o) o->*r.option = v != nullptr; break;
            case KNOB_OPTION_COUNT: if (o) o->*r.option = atol(v ? v : r.dflt); break;
        }
    }
    if (!k) return;
    // coupled defaults
    if (k->gn_no_fold && !getenv("LNS_GN_FUSE_MIN_HW")) k->gn_fuse_min_hw = 1024;
    if (k->up2_resident) k->up2_quad = false;
    if (k->wgrad_target_blocks < 1) k->wgrad_target_blocks = 512;
    if (k->wgrad_max_slices < 1) k->wgrad_max_slices = 128;
}

inline const Knobs& knobs() {
    static const Knobs k = [] { Knobs t{}; parse_knob_rows(&t, nullptr); return t; }();
    return k;
}
inline OptionDefaults option_defaults() {
    OptionDefaults o{};
    parse_knob_rows(nullptr, &o);
    return o;
}

}  // namespace lns

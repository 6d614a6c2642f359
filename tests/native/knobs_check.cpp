// Stand-alone host check of the switch table (csrc/lns_knobs.h) and of the form rules that planner and launcher share
// (attn_is_f16, fa_sandwich_form in csrc/lns_kernels.h).  Links the built library for the two rules, calls host functions only
// (no GPU, no HIP call); built and run by tests/test_knobs_cpu.py, one child process per environment.
//   knobs_check rows    one line per row: name, kind, default text, meaning (tab-separated)
//   knobs_check values  one line per row: name and the value parsed from this process's environment
//   knobs_check once    values of a flag, a count and an option default; then the three are set and the values printed again
//   knobs_check forms   the two rules on the launcher's five plane tilings and on a 96 x 192 plane, with and without amax
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "lns_kernels.h"
#include "lns_knobs.h"

using namespace lns;

static void print_values(const Knobs& k, const OptionDefaults& o) {
    for (const KnobRow& r : kKnobRows) {
        switch (r.kind) {
            case KNOB_FLAG: printf("%s %d\n", r.env, (int)(k.*r.flag)); break;
            case KNOB_COUNT: printf("%s %ld\n", r.env, k.*r.count); break;
            case KNOB_CONV3_SPLIT: printf("%s %s\n", r.env, k.conv3_split == CONV3_SPLIT_BF16X3 ? "bf16x3" : "f16x2"); break;
            case KNOB_OPTION_FLAG:
            case KNOB_OPTION_COUNT: printf("%s %ld\n", r.env, o.*r.option); break;
        }
    }
}

static void print_once() {
    const OptionDefaults o = option_defaults();
    printf("LNS_GN_NO_FUSE %d LNS_FA_PPB %ld LNS_DECODE_GROUP %ld\n", (int)knobs().gn_no_fuse, knobs().fa_ppb, o.decode_group);
}

static const char* sandwich_name(FaSandwichForm f) {
    switch (f) {
        case FA_SAND_F16X2: return "f16x2";
        case FA_SAND_BF16X3: return "bf16x3";
        case FA_SAND_BF16X3_3WAVE: return "bf16x3_3wave";
        case FA_SAND_FP32: return "fp32";
        default: return "none";
    }
}

int main(int argc, char** argv) {
    const char* mode = argc > 1 ? argv[1] : "";
    if (!strcmp(mode, "rows")) {
        for (const KnobRow& r : kKnobRows) printf("%s\t%s\t%s\t%s\n", r.env, knob_kind_name(r.kind), r.dflt, r.doc);
    } else if (!strcmp(mode, "values")) {
        print_values(knobs(), option_defaults());
    } else if (!strcmp(mode, "once")) {
        print_once();
        setenv("LNS_GN_NO_FUSE", "1", 1);
        setenv("LNS_FA_PPB", "8", 1);
        setenv("LNS_DECODE_GROUP", "5", 1);
        print_once();
    } else if (!strcmp(mode, "forms")) {
        const int planes[6][2] = {{32, 32}, {32, 64}, {64, 64}, {64, 96}, {64, 32}, {96, 192}};
        unsigned amax = 0;
        for (const int* p : planes)
            for (int with_amax = 0; with_amax < 2; ++with_amax) {
                FaSandwichArgs fs;
                memset(&fs, 0, sizeof fs);
                fs.B = 2; fs.heads = 4; fs.C = 64; fs.H = p[0]; fs.W = p[1];
                fs.amax_u = with_amax ? &amax : nullptr;
                AttnArgs at;
                memset(&at, 0, sizeof at);
                at.B = 2; at.heads = 4; at.D = 32; at.n = p[0] * p[1];
                at.amax_in = with_amax ? &amax : nullptr;
                printf("%dx%d amax %d: sandwich %s attn_f16 %d\n", p[0], p[1], with_amax, sandwich_name(fa_sandwich_form(fs)), (int)attn_is_f16(at));
            }
    } else {
        fprintf(stderr, "usage: knobs_check rows|values|once|forms\n");
        return 2;
    }
    printf("ALL DONE\n");
    return 0;
}

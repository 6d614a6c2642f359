// Stand-alone host check of the plan's tagged pointers (csrc/lns_resolve.h and the pointer lists of csrc/lns_kernels.h).
// No GPU and no HIP call: built with the host compiler under AddressSanitizer + UBSan by tests/test_resolve_cpu.py.
// Every listed pointer of every argument block, and of every op type, goes through the same cases; the program prints how
// many pointers / strides each visitor walks (the Python test pins them) and "ALL OK" at the end.
#include <cstdio>
#include <cstring>
#include <type_traits>

#include "lns_resolve.h"

using namespace lns;

static int g_fail = 0;
#define CHECK(cond, ...)                                                  \
    do {                                                                  \
        if (!(cond)) {                                                    \
            ++g_fail;                                                     \
            printf("FAIL %s:%d %s | ", __FILE__, __LINE__, #cond);        \
            printf(__VA_ARGS__);                                          \
            printf("\n");                                                 \
        }                                                                 \
    } while (0)

// real host buffers stand in for the device regions: nothing is dereferenced, every address is a valid one
static char g_ws[4096], g_wt[4096], g_ct[4096], g_ext[EX_COUNT][4096], g_plain[4096];
static const size_t OFF = 0x230, INT_BYTES = 64;

static Bases bases() {
    Bases B = {};
    B.b[SP_WS] = g_ws; B.b[SP_WT] = g_wt; B.b[SP_CT] = g_ct;
    for (int i = 0; i < EX_COUNT; ++i) { B.b[SP_EXT0 + i] = g_ext[i]; B.bs[SP_EXT0 + i] = 1000 + i; B.bs2[SP_EXT0 + i] = 2000 + i; }
    return B;
}

template <class V> static int count_ptrs(V& v) { int n = 0; for_each_ptr(v, [&](auto*&) { ++n; }); return n; }
template <class V> static int count_strides(V& v) { int n = 0; for_each_stride(v, [&](long&) { ++n; }); return n; }
template <class V> static void set_ptr(V& v, int i, uint64_t val) {
    int n = 0;
    for_each_ptr(v, [&](auto*& p) { if (n++ == i) p = as_ptr<std::remove_pointer_t<std::remove_reference_t<decltype(p)>>>(val); });
}
template <class V> static uint64_t get_ptr(V& v, int i) {
    int n = 0; uint64_t r = ~0ull;
    for_each_ptr(v, [&](auto*& p) { if (n++ == i) r = reinterpret_cast<uint64_t>(p); });
    return r;
}
static uint64_t addr(const char* base, size_t off = 0) { return reinterpret_cast<uint64_t>(base) + off; }

// resolution of a whole holder: an argument block through resolve(), an Op through its pointer walk
template <class A> static bool run_resolve(A& a, const Bases& B) { return resolve(a, B); }
static bool run_resolve(Op& op, const Bases& B) { for_each_ptr(op, [&](auto*& p) { fix(p, B); }); return !B.bad; }

// the cases every listed pointer goes through; make() returns a zeroed holder (block, or Op of one type)
template <class Make> static void check_pointers(const char* name, Make make) {
    auto probe = make();
    const int n = count_ptrs(probe);
    struct { int space; const char* base; } good[] = {{SP_WS, g_ws}, {SP_WT, g_wt}, {SP_CT, g_ct}, {SP_EXT0 + EX_IN, g_ext[EX_IN]},
                                                       {SP_EXT0 + EX_SS, g_ext[EX_SS]}};
    for (int i = 0; i < n; ++i) {
        for (auto& g : good) {                                   // workspace / weight / constant / external tag -> base + offset
            auto a = make(); Bases B = bases();
            set_ptr(a, i, tag(g.space, OFF));
            CHECK(run_resolve(a, B) && !B.bad, "%s ptr %d space %d", name, i, g.space);
            CHECK(get_ptr(a, i) == addr(g.base, OFF), "%s ptr %d space %d", name, i, g.space);
            for (int j = 0; j < n; ++j) CHECK(j == i || get_ptr(a, j) == 0, "%s ptr %d: ptr %d moved", name, i, j);   // null stays null
        }
        {                                                        // a plain device address is untouched
            auto a = make(); Bases B = bases();
            set_ptr(a, i, addr(g_plain, 16));
            CHECK(run_resolve(a, B) && get_ptr(a, i) == addr(g_plain, 16), "%s ptr %d plain", name, i);
        }
        // refused, pointer nulled, bad set: a space without a base (an unused external slot, a space id past the table), and a
        // constant-blob tag that still carries a segment bit
        const uint64_t refused[] = {tag(SP_EXT0 + 7, OFF), tag(0x20, OFF), tag(SP_CT, OFF) | CT_FLOAT_SEG, tag(SP_CT, OFF) | CT_INT_SEG,
                                    tag(SP_CT, OFF) | CT_FLOAT_SEG | CT_INT_SEG};
        for (uint64_t t : refused) {
            auto a = make(); Bases B = bases();
            set_ptr(a, i, t);
            CHECK(!run_resolve(a, B) && B.bad, "%s ptr %d tag %llx accepted", name, i, (unsigned long long)t);
            CHECK(get_ptr(a, i) == 0, "%s ptr %d tag %llx not nulled", name, i, (unsigned long long)t);
        }
        {                                                        // still tagged after resolution (here: the base itself is a tag)
            auto a = make(); Bases B = bases();
            B.b[SP_WS] = reinterpret_cast<char*>(tag(SP_WT, 0x1000));
            set_ptr(a, i, tag(SP_WS, OFF));
            CHECK(!run_resolve(a, B) && B.bad, "%s ptr %d left tagged but reported resolved", name, i);
        }
        {                                                        // rebase: int segment same offset, float segment + int bytes, bits cleared
            auto a = make(); Bases B = bases();
            set_ptr(a, i, tag(SP_CT, OFF) | CT_INT_SEG);
            for_each_ptr(a, [&](auto*& p) { rebase_const(p, INT_BYTES); });
            CHECK(get_ptr(a, i) == tag(SP_CT, OFF), "%s ptr %d int rebase", name, i);
            CHECK(run_resolve(a, B) && get_ptr(a, i) == addr(g_ct, OFF), "%s ptr %d int rebase resolve", name, i);
            a = make(); B = bases();
            set_ptr(a, i, tag(SP_CT, OFF) | CT_FLOAT_SEG);
            for_each_ptr(a, [&](auto*& p) { rebase_const(p, INT_BYTES); });
            CHECK(get_ptr(a, i) == tag(SP_CT, OFF + INT_BYTES), "%s ptr %d float rebase", name, i);
            CHECK(run_resolve(a, B) && get_ptr(a, i) == addr(g_ct, OFF + INT_BYTES), "%s ptr %d float rebase resolve", name, i);
            for (uint64_t keep : {tag(SP_WS, OFF), tag(SP_EXT0 + EX_OUT, 0), addr(g_plain, 32)}) {   // anything else: left alone
                a = make();
                set_ptr(a, i, keep);
                for_each_ptr(a, [&](auto*& p) { rebase_const(p, INT_BYTES); });
                CHECK(get_ptr(a, i) == keep, "%s ptr %d rebase touched %llx", name, i, (unsigned long long)keep);
            }
        }
    }
    {                                                            // all pointers tagged at once: none keeps a top byte
        auto a = make(); Bases B = bases();
        for (int i = 0; i < n; ++i) set_ptr(a, i, tag(good[i % 5].space, OFF + 16 * i));
        CHECK(run_resolve(a, B), "%s all tagged", name);
        for (int i = 0; i < n; ++i) {
            CHECK(untagged(reinterpret_cast<const void*>(get_ptr(a, i))), "%s ptr %d top byte", name, i);
            CHECK(get_ptr(a, i) == addr(good[i % 5].base, OFF + 16 * i), "%s ptr %d all tagged", name, i);
        }
    }
}

template <class A> static void check_block(const char* name) {
    A probe = {};
    printf("ptrs %s %d\nstrides %s %d\n", name, count_ptrs(probe), name, count_strides(probe));
    check_pointers(name, [] { A a = {}; return a; });
    const int ns = count_strides(probe);
    for (int j = 0; j < ns; ++j)
        for (int slot = 0; slot < EX_COUNT; ++slot) {            // a negative batch stride is its external slot's stride
            A a = {}; Bases B = bases();
            int n = 0;
            for_each_stride(a, [&](long& bs) { bs = (n++ == j) ? -(long)(slot + 1) : 77; });
            CHECK(resolve(a, B), "%s stride %d", name, j);
            n = 0;
            for_each_stride(a, [&](long& bs) { CHECK(bs == ((n == j) ? 1000 + slot : 77), "%s stride %d slot %d: %ld", name, j, slot, bs); ++n; });
        }
}

static void check_conv_rules() {
    {   // an input on a two-level external slot is refused
        ConvArgs a = {}; Bases B = bases();
        B.bdiv[SP_EXT0 + EX_IN] = 4;
        a.x = as_ptr<const float>(tag(SP_EXT0 + EX_IN, 0)); a.x_bs = -(long)(EX_IN + 1);
        CHECK(!resolve_conv(a, B) && B.bad, "conv input on a two-level slot accepted");
    }
    {   // an output on one takes the slot's second level over
        ConvArgs a = {}; Bases B = bases();
        B.bdiv[SP_EXT0 + EX_OUT] = 4;
        a.x = as_ptr<const float>(tag(SP_EXT0 + EX_IN, 0)); a.x_bs = -(long)(EX_IN + 1);
        a.y = as_ptr<float>(tag(SP_EXT0 + EX_OUT, 0)); a.y_bs = -(long)(EX_OUT + 1);
        CHECK(resolve_conv(a, B), "conv output on a two-level slot refused");
        CHECK(a.y_bdiv == 4 && a.y_bs2 == 2000 + EX_OUT && a.y_bs == 1000 + EX_OUT && a.x_bs == 1000 + EX_IN, "conv two-level hand-over");
        CHECK(reinterpret_cast<uint64_t>(a.y) == addr(g_ext[EX_OUT]), "conv y");
    }
    {   // a plain output keeps what the planner wrote
        ConvArgs a = {}; Bases B = bases();
        a.y_bs = 512; a.y_bdiv = 0; a.y_bs2 = 0;
        CHECK(resolve_conv(a, B) && a.y_bs == 512 && a.y_bdiv == 0 && a.y_bs2 == 0, "conv plain output");
    }
}

static void check_ops() {
    static const struct { OpType t; const char* name; } types[] = {
        {OP_CONV, "OP_CONV"}, {OP_GNSTATS, "OP_GNSTATS"}, {OP_LNPE, "OP_LNPE"}, {OP_ATTN, "OP_ATTN"}, {OP_FAPOOL, "OP_FAPOOL"},
        {OP_FARED, "OP_FARED"}, {OP_FARED2, "OP_FARED2"}, {OP_FALRK, "OP_FALRK"}, {OP_FALRK2, "OP_FALRK2"}, {OP_FASAND, "OP_FASAND"},
        {OP_FAGSPLIT, "OP_FAGSPLIT"}, {OP_FAFUSED, "OP_FAFUSED"}, {OP_CONDBASE, "OP_CONDBASE"}, {OP_CONDBLK, "OP_CONDBLK"},
        {OP_APPLY, "OP_APPLY"}, {OP_SPECTRAL, "OP_SPECTRAL"}, {OP_FCOMBINE, "OP_FCOMBINE"}, {OP_VECLIN, "OP_VECLIN"}, {OP_TRACE, "OP_TRACE"}};
    for (const auto& ty : types) {
        auto make = [&] { Op op; op.type = ty.t; return op; };
        Op probe = make();
        printf("op %s %d\n", ty.name, count_ptrs(probe));
        check_pointers(ty.name, make);
    }
}

int main() {
    check_block<ConvArgs>("ConvArgs");
    check_block<GnStatsArgs>("GnStatsArgs");
    check_block<LnPeArgs>("LnPeArgs");
    check_block<AttnArgs>("AttnArgs");
    check_block<FaPoolArgs>("FaPoolArgs");
    check_block<FaReducerArgs>("FaReducerArgs");
    check_block<FaLrkArgs>("FaLrkArgs");
    check_block<FaSandwichArgs>("FaSandwichArgs");
    check_block<FaGsplitArgs>("FaGsplitArgs");
    check_block<FaFusedArgs>("FaFusedArgs");
    check_block<CondBaseArgs>("CondBaseArgs");
    check_block<CondBlockArgs>("CondBlockArgs");
    check_block<ApplyArgs>("ApplyArgs");
    check_block<SpectralArgs>("SpectralArgs");
    check_block<FourierCombineArgs>("FourierCombineArgs");
    check_block<VecLinearArgs>("VecLinearArgs");
    check_conv_rules();
    check_ops();
    if (g_fail) { printf("%d FAILED\n", g_fail); return 1; }
    printf("ALL OK\n");
    return 0;
}

// Tagged pointers of a launch plan (host only: no HIP call, a plain host compiler can include this).
// The planner writes (space << 56) | byte offset into the pointer members of an op's argument blocks; Planner::finish()
// rebases the constant-blob tags, Runner::run resolves a copy of the block immediately before its launch.  Both walk the
// pointer lists next to the blocks (for_each_ptr / for_each_stride, lns_kernels.h) and the per-op dispatch below.
#pragma once
#include <stdexcept>

#include "lns_engine.h"

namespace lns {

inline uint64_t tag(int space, size_t byte_off) { return ((uint64_t)space << 56) | (uint64_t)byte_off; }
template <class T> inline T* as_ptr(uint64_t t) { return reinterpret_cast<T*>(t); }
// SP_CT tags carry their segment of the constant blob until finish() has rebased them: ints first, then floats
constexpr uint64_t CT_INT_SEG = 1ull << 55, CT_FLOAT_SEG = 1ull << 54, TAG_OFFSET = (1ull << 56) - 1;

struct Bases { char* b[16]; long bs[16]; long bs2[16]; int bdiv[16]; mutable bool bad = false; };
inline bool untagged(const void* p) { return (reinterpret_cast<uint64_t>(p) >> 56) == 0; }
// tag -> device address.  A pointer that reached a launch still tagged would be a wild device address (the GPU abort of round 1,
// DESIGN.md "FUSE2 abort"): whatever does not resolve, or still has a top byte afterwards, sets `bad`, and false means "do not launch"
// (the result is `!bad` of the whole Bases -- has anything failed so far -- not a verdict on this one pointer)
template <class T> inline bool fix(T*& p, const Bases& B) {
    const uint64_t v = reinterpret_cast<uint64_t>(p);
    const int sp = (int)(v >> 56);
    if (sp == SP_NULL) return !B.bad;                                                // null, or already a device address
    if (sp >= 16 || !B.b[sp]) { B.bad = true; p = nullptr; return false; }           // tag without a base: never launch on it
    if (sp == SP_CT && (v & (CT_INT_SEG | CT_FLOAT_SEG))) { B.bad = true; p = nullptr; return false; }   // constant finish() did not rebase
    p = reinterpret_cast<T*>(B.b[sp] + (v & TAG_OFFSET));
    if (!untagged(p)) B.bad = true;
    return !B.bad;
}
inline void fixbs(long& bs, const Bases& B) {
    if (bs < 0) bs = B.bs[SP_EXT0 + (int)(-bs - 1)];
}
// every listed pointer and tagged batch stride of one argument block (for_each_ptr / for_each_stride next to the block)
template <class A> inline bool resolve(A& a, const Bases& B) {
    for_each_ptr(a, [&](auto*& p) { fix(p, B); });
    for_each_stride(a, [&](long& bs) { fixbs(bs, B); });
    return !B.bad;
}
// the convolution: an output handed in by the caller may be addressed in two levels (step-batched decode), an input never
inline bool resolve_conv(ConvArgs& a, const Bases& B) {
    if (a.y_bs < 0) {
        const int sl = SP_EXT0 + (int)(-a.y_bs - 1);
        a.y_bs2 = B.bs2[sl]; a.y_bdiv = B.bdiv[sl];
    }
    if (a.x_bs < 0 && B.bdiv[SP_EXT0 + (int)(-a.x_bs - 1)]) B.bad = true;
    return resolve(a, B);
}

// constant-blob tag -> its offset in the uploaded blob (int_bytes of ints, then the floats); anything else is left alone
template <class T> inline void rebase_const(T*& p, size_t int_bytes) {
    const uint64_t v = reinterpret_cast<uint64_t>(p);
    if ((v >> 56) != SP_CT) return;
    p = as_ptr<T>(tag(SP_CT, (v & TAG_OFFSET & ~(CT_INT_SEG | CT_FLOAT_SEG)) + ((v & CT_FLOAT_SEG) ? int_bytes : 0)));
}

// every pointer an op of this type hands to its launch (a block the op does not use is all null and not visited)
template <class F> void for_each_ptr(Op& op, F&& f) {
    switch (op.type) {
        case OP_CONV: for_each_ptr(op.conv, f); return;
        case OP_GNSTATS: for_each_ptr(op.gn, f); f(op.gn_tile_part); return;
        case OP_LNPE: for_each_ptr(op.ln, f); return;
        case OP_ATTN: for_each_ptr(op.at, f); return;
        case OP_FAPOOL: for_each_ptr(op.fp, f); return;
        case OP_FARED2: for_each_ptr(op.fr2, f); [[fallthrough]];
        case OP_FARED: for_each_ptr(op.fr, f); return;
        case OP_FALRK2: for_each_ptr(op.fl2, f); [[fallthrough]];
        case OP_FALRK: for_each_ptr(op.fl, f); return;
        case OP_FASAND: for_each_ptr(op.fs, f); return;
        case OP_FAGSPLIT: for_each_ptr(op.fg, f); return;
        case OP_FAFUSED: for_each_ptr(op.ff, f); return;
        case OP_CONDBASE: for_each_ptr(op.cb, f); return;
        case OP_CONDBLK: for_each_ptr(op.ck, f); return;
        case OP_APPLY: for_each_ptr(op.ap, f); return;
        case OP_SPECTRAL: for_each_ptr(op.sp, f); return;
        case OP_FCOMBINE: for_each_ptr(op.fc, f); return;
        case OP_VECLIN: for_each_ptr(op.vl, f); return;
        case OP_TRACE: { const float* p = as_ptr<const float>(op.t_ptr); f(p); op.t_ptr = reinterpret_cast<uint64_t>(p); return; }
    }   // (no default: -Wswitch names a missing op type at compile time)
    throw std::logic_error("for_each_ptr(Op&): op type without a case: " + op.name);   // finish() would skip its rebase
}

}  // namespace lns

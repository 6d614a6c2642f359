// Stand-alone host check of OpScratch (csrc/lns_op_scratch.h), the owner of an op-level entry point's device memory.
// The five HIP calls it makes are defined here: counting, malloc-backed stand-ins, of which call number `fail_at` (1-based, in
// issue order) fails.  Links neither the library nor the HIP runtime; built with the address and undefined-behaviour sanitizers
// and run by tests/test_op_scratch_cpu.py, once without a failure and once per call position.
//
// The sequence: two uploads, the amax words, a NaN-filled allocation, finish -- 4 allocations, 2 copies, 2 fills, 1 wait.
// One line per run: what was issued, what came back, and whether every rule held ("ok 1").
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>

#define LNS_AMAX_SUB 16        // lns_kernels.h's
#include "lns_op_scratch.h"

namespace {
int calls = 0, fail_at = 0;                    // every stand-in counts; call number fail_at fails
int n_malloc = 0, n_copy = 0, n_fill = 0, n_sync = 0, n_free = 0, frees_before_sync = 0, issued_after_error = 0, double_free = 0;
bool failed = false;
hipError_t failed_with = hipSuccess;
std::set<void*> live;

hipError_t step(hipError_t on_failure, bool transfers) {
    ++calls;
    if (failed && transfers) ++issued_after_error;
    if (calls != fail_at) return hipSuccess;
    failed = true;
    failed_with = on_failure;
    return on_failure;
}
}  // namespace

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) {
    ++n_malloc;
    if (hipError_t e = step(hipErrorOutOfMemory, true)) { *p = reinterpret_cast<void*>(0x10); return e; }   // a pointer that must not be kept
    *p = malloc(bytes);
    live.insert(*p);
    return hipSuccess;
}
hipError_t hipFree(void* p) {
    ++n_free;
    if (!n_sync) ++frees_before_sync;
    if (!live.erase(p)) { ++double_free; return hipErrorInvalidValue; }
    free(p);
    return hipSuccess;
}
hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind) {
    ++n_copy;
    if (hipError_t e = step(hipErrorInvalidValue, true)) return e;
    memcpy(dst, src, bytes);
    return hipSuccess;
}
hipError_t hipMemsetAsync(void* dst, int value, size_t bytes, hipStream_t) {
    ++n_fill;
    if (hipError_t e = step(hipErrorLaunchFailure, true)) return e;
    memset(dst, value, bytes);
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t) {
    ++n_sync;
    return step(hipErrorIllegalAddress, false);
}
}

int main(int argc, char** argv) {
    fail_at = argc > 1 ? atoi(argv[1]) : 0;
    const int B = 3;
    const float host[5] = {1.0f, 2.0f, 3.0f, 4.0f, 5.0f};
    const std::vector<float> vec(7, 0.5f);
    hipError_t got = hipSuccess;
    bool nulls_after_error = true, data_ok = true;
    size_t held = 0;
    {
        lns::OpScratch sc;
        void* p[4];
        bool before[4];
        before[0] = failed; p[0] = sc.upload(host, 5);
        before[1] = failed; p[1] = sc.upload(vec);
        before[2] = failed; p[2] = sc.amax_words(B, nullptr);
        before[3] = failed; p[3] = sc.alloc(9);
        sc.fill(p[3], 0xFF, 9, nullptr);
        for (int i = 0; i < 4; ++i) {
            if (before[i] && p[i]) nulls_after_error = false;         // asked for after the failure
            if (p[i] && !live.count(p[i])) nulls_after_error = false;      // (the failed hipMalloc's own pointer is not handed out)
        }
        if (!fail_at) {
            unsigned ff;
            memset(&ff, 0xFF, 4);
            data_ok = !memcmp(p[0], host, sizeof host) && !memcmp(p[1], vec.data(), 7 * 4) && static_cast<unsigned*>(p[2])[B * LNS_AMAX_SUB - 1] == 0u &&
                      static_cast<unsigned*>(p[3])[8] == ff;
        }
        got = sc.finish(nullptr);
        held = live.size();
        if (sc.finish(nullptr) != got) data_ok = false;               // the first error stays the answer
    }
    const size_t mallocs_ok = (size_t)n_malloc - (failed && failed_with == hipErrorOutOfMemory ? 1 : 0);
    const bool ok = live.empty() && !double_free && (size_t)n_free == mallocs_ok && held == mallocs_ok && got == failed_with &&
                    !issued_after_error && !frees_before_sync && n_sync == 2 && nulls_after_error && data_ok;
    printf("fail_at %d: malloc %d copy %d fill %d sync %d free %d leaked %zu double_free %d after_error %d frees_before_sync %d "
           "returned %d injected %d nulls_after_error %d ok %d\n", fail_at, n_malloc, n_copy, n_fill, n_sync, n_free, live.size(), double_free,
           issued_after_error, frees_before_sync, (int)got, (int)failed_with, (int)nulls_after_error, (int)ok);
    return ok ? 0 : 1;
}

// Device memory an op-level entry point (lns_ops.inc) owns for the length of one call.  The first failure sticks: after it
// every allocation returns null and no copy or fill is issued; finish() waits for the stream, so nothing is freed under a
// kernel that may still run, and returns that first failure.  Needs LNS_AMAX_SUB (lns_kernels.h) defined by the includer.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstring>
#include <vector>

namespace lns {

// max |.| of a sample as a float: the maximum over the sample's sub-words (amax_load), words [B][LNS_AMAX_SUB] device ->
// dev_out [B] device
inline hipError_t amax_words_to_float(const unsigned* words, int B, float* dev_out) {
    std::vector<unsigned> hw((size_t)B * LNS_AMAX_SUB);
    std::vector<float> hm(B);
    if (hipError_t err = hipMemcpy(hw.data(), words, hw.size() * 4, hipMemcpyDeviceToHost)) return err;
    for (int b = 0; b < B; ++b) {
        unsigned m = 0u;
        for (int k = 0; k < LNS_AMAX_SUB; ++k) m = std::max(m, hw[(size_t)b * LNS_AMAX_SUB + k]);
        memcpy(&hm[b], &m, 4);
    }
    return hipMemcpy(dev_out, hm.data(), (size_t)B * 4, hipMemcpyHostToDevice);
}

struct OpScratch {
    std::vector<void*> ptrs;
    hipError_t err = hipSuccess;
    OpScratch() = default;
    OpScratch(const OpScratch&) = delete;
    OpScratch& operator=(const OpScratch&) = delete;
    ~OpScratch() { release(); }

    bool ok() const { return err == hipSuccess; }
    bool note(hipError_t e) { if (ok()) err = e; return ok(); }    // a launch's or a copy's result: the first failure is kept
    void* alloc(size_t words) {                                    // 4-byte words
        void* p = nullptr;
        if (!ok() || !note(hipMalloc(&p, std::max<size_t>(words, 1) * 4))) return nullptr;
        ptrs.push_back(p);
        return p;
    }
    void copy_in(void* dev, const void* host, size_t words) {      // blocking
        if (ok()) note(hipMemcpy(dev, host, words * 4, hipMemcpyHostToDevice));
    }
    void fill(void* dev, int byte, size_t words, hipStream_t s) {  // in stream order
        if (ok()) note(hipMemsetAsync(dev, byte, words * 4, s));
    }
    float* upload(const std::vector<float>& host) { return upload(host.data(), host.size()); }
    float* upload(const float* host, size_t count) {
        float* p = static_cast<float*>(alloc(count));
        copy_in(p, host, count);
        return p;
    }
    unsigned* amax_words(int B, hipStream_t s) {                   // [B][LNS_AMAX_SUB], zeroed in stream order
        unsigned* p = static_cast<unsigned*>(alloc((size_t)B * LNS_AMAX_SUB));
        fill(p, 0, (size_t)B * LNS_AMAX_SUB, s);
        return p;
    }
    // the end of a call, with or without a failure: nothing of this call runs on the stream after it
    hipError_t finish(hipStream_t s) { note(hipStreamSynchronize(s)); return err; }
    // frees now (a long-lived owner that prepares again); the destructor's work
    void release() { for (void* p : ptrs) (void)hipFree(p); ptrs.clear(); err = hipSuccess; }
};

}  // namespace lns

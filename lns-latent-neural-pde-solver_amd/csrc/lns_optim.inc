// ---------------------------------------------------------------------------------------------------------------------
// Loss and optimiser kernels of the device-resident stage-2 training step  (included by lns_train_kernels.hip)
//
// Reference: the three lines around the training rollout, train_stage2_ns2d.py:213-216
//     loss = model(z_in, z_out, F.smooth_l1_loss) ; loss.backward() ; optim.step()      (torch.optim.Adam, :179)
//   * smooth_l1_kernel / smooth_l1_finish_kernel: F.smooth_l1_loss(pred, target, reduction='mean', beta) and its gradient
//     w.r.t. pred in ONE pass over both tensors.  A block owns a fixed chunk of SL1_CHUNK elements whatever the grid, a
//     thread a fixed set of them, and the sums are combined in a fixed tree: the loss is bit-reproducible and does not
//     depend on how the blocks are scheduled.  No float atomics.
//   * adam_multi_kernel: torch.optim.Adam's update (no amsgrad, L2 weight decay added to the gradient) of MANY tensors
//     in one launch.  The table (four pointers and a length per tensor) travels in the kernel-argument block, a block
//     finds its tensor by a binary search over the tensors' first chunk numbers.
//   * grad_sumsq_multi_kernel / grad_norm_finish_kernel: torch.nn.utils.clip_grad_norm_'s global L2 norm and clip coefficient
//     of MANY gradient tensors (same table scheme), summed in double in a fixed order; update_multi_kernel: Adam / AdamW on
//     the clipped gradient, the coefficient read from the device.  Not in the reference's loop: see include/lns.h.
// All are memory-bound elementwise kernels: 16-byte accesses where the pointers allow it, one read of every input.
// ---------------------------------------------------------------------------------------------------------------------

// ---- smooth L1 ------------------------------------------------------------------------------------------------------
// SL1_CHUNK = 256 threads x SL1_ITERS x 4 elements (lns.h: LNS_SL1_CHUNK)
constexpr int SL1_ITERS = 4;
static_assert(SL1_CHUNK == 256 * SL1_ITERS * 4, "chunk = threads x iterations x vector width");

__device__ __forceinline__ float sl1_term(float p, float t, float beta, float half_inv_beta, float scale_q, float scale_l, float& g) {
    const float d = p - t;
    const float ad = fabsf(d);
    const bool quad = ad < beta;
    // gradient: d / (beta N) inside, sign(d) / N outside; both factors are rounded once on the host from double
    // (a NaN difference is in neither half-line: it goes through the product and stays NaN, as in torch)
    g = quad ? d * scale_q : (d > 0.0f ? scale_l : (d < 0.0f ? -scale_l : d * scale_q));
    return quad ? d * d * half_inv_beta : ad - 0.5f * beta;
}

// fixed-order sum of one value per thread of a 256-thread block, in double (a few hundred adds: free beside the loads)
__device__ __forceinline__ double block_sum256(double v, double* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(256) void smooth_l1_kernel(const float* __restrict__ pred, const float* __restrict__ target, long n,
                                                        float beta, float half_inv_beta, float scale_q, float scale_l,
                                                        float* __restrict__ grad, float* __restrict__ partial, int vec) {
    __shared__ double red[256];
    const long base = (long)blockIdx.x * SL1_CHUNK;
    float acc = 0.0f;                                   // 16 terms per thread, then the tree in double
#pragma unroll
    for (int j = 0; j < SL1_ITERS; ++j) {
        const long i = base + ((long)j * 256 + threadIdx.x) * 4;
        if (vec && i + 3 < n) {
            const float4 p = *reinterpret_cast<const float4*>(pred + i);
            const float4 t = *reinterpret_cast<const float4*>(target + i);
            float4 g;
            const float l0 = sl1_term(p.x, t.x, beta, half_inv_beta, scale_q, scale_l, g.x);
            const float l1 = sl1_term(p.y, t.y, beta, half_inv_beta, scale_q, scale_l, g.y);
            const float l2 = sl1_term(p.z, t.z, beta, half_inv_beta, scale_q, scale_l, g.z);
            const float l3 = sl1_term(p.w, t.w, beta, half_inv_beta, scale_q, scale_l, g.w);
            acc += (l0 + l1) + (l2 + l3);
            if (grad) *reinterpret_cast<float4*>(grad + i) = g;
        } else {
            // tail of the tensor, or pointers that are not 16-byte aligned: the same elements, the same order of additions
            float l[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (i + k < n) {
                    float g;
                    l[k] = sl1_term(pred[i + k], target[i + k], beta, half_inv_beta, scale_q, scale_l, g);
                    if (grad) grad[i + k] = g;
                }
            }
            acc += (l[0] + l[1]) + (l[2] + l[3]);
        }
    }
    const double s = block_sum256((double)acc, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = (float)s;
}

// one block: partial sums in a fixed order -> the mean, one float on the device
__global__ __launch_bounds__(256) void smooth_l1_finish_kernel(const float* __restrict__ partial, int n_partial, double inv_n,
                                                               float* __restrict__ loss_out) {
    __shared__ double red[256];
    double a = 0.0;
    for (int i = threadIdx.x; i < n_partial; i += 256) a += (double)partial[i];
    const double s = block_sum256(a, red);
    if (threadIdx.x == 0) *loss_out = (float)(s * inv_n);
}

long smooth_l1_partials(long n) { return (n + SL1_CHUNK - 1) / SL1_CHUNK; }

hipError_t launch_smooth_l1(const float* pred, const float* target, long n, float beta, float* loss_out, float* grad, float* partial,
                            hipStream_t s) {
    const long blocks = smooth_l1_partials(n);
    const double inv_n = 1.0 / (double)n;
    const int vec = ((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(target) | reinterpret_cast<uintptr_t>(grad)) & 15) == 0;
    hipLaunchKernelGGL(smooth_l1_kernel, dim3((unsigned)blocks), dim3(256), 0, s, pred, target, n, beta, (float)(0.5 / (double)beta),
                       (float)(inv_n / (double)beta), (float)inv_n, grad, partial, vec);
    hipError_t rc = hipGetLastError();
    if (rc != hipSuccess) return rc;
    hipLaunchKernelGGL(smooth_l1_finish_kernel, dim3(1), dim3(256), 0, s, partial, (int)blocks, inv_n, loss_out);
    return hipGetLastError();
}

// ---- multi-tensor Adam ----------------------------------------------------------------------------------------------
// A block owns ADAM_CHUNK consecutive elements of ONE tensor; tensor i owns the chunk numbers [first_i, first_{i+1}).
constexpr int ADAM_CHUNK = 2048;          // 256 threads x 2 x 16 bytes per array
struct AdamTable {
    float step_size;                      // lr / (1 - beta1^t)
    float beta1, one_minus_beta1, beta2, one_minus_beta2;
    float bc2_sqrt;                       // sqrt(1 - beta2^t)
    float eps, weight_decay;
    int count, pad;
    AdamTensor t[ADAM_MAX_TENSORS];       // 40 bytes each: the whole argument block stays under the 4 KB limit
};
static_assert(sizeof(AdamTensor) == 40, "four pointers, a length and a first chunk");
static_assert(sizeof(AdamTable) <= 4096 - 64, "kernel-argument block limit");

__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, const AdamTable& a) {
    g = a.weight_decay != 0.0f ? g + a.weight_decay * p : g;
    m = a.beta1 * m + a.one_minus_beta1 * g;
    v = a.beta2 * v + a.one_minus_beta2 * (g * g);
    const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
    p = p - a.step_size * (m / denom);
}

__global__ __launch_bounds__(256) void adam_multi_kernel(const AdamTable a) {
    // the tensor of this block: last i with t[i].first <= blockIdx.x (uniform over the block: scalar loads of the table)
    int lo = 0, hi = a.count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.t[mid].first <= blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const AdamTensor t = a.t[lo];
    const unsigned off = (blockIdx.x - t.first) * (unsigned)ADAM_CHUNK;
    const unsigned n = t.n;
    const bool vec = ((reinterpret_cast<uintptr_t>(t.p) | reinterpret_cast<uintptr_t>(t.g) | reinterpret_cast<uintptr_t>(t.m) |
                       reinterpret_cast<uintptr_t>(t.v)) & 15) == 0;
#pragma unroll
    for (int j = 0; j < ADAM_CHUNK / 1024; ++j) {
        const unsigned i = off + ((unsigned)j * 256 + threadIdx.x) * 4;
        if (i >= n) break;
        if (vec && i + 3 < n) {
            float4 p = *reinterpret_cast<const float4*>(t.p + i);
            const float4 g = *reinterpret_cast<const float4*>(t.g + i);
            float4 m = *reinterpret_cast<const float4*>(t.m + i);
            float4 v = *reinterpret_cast<const float4*>(t.v + i);
            adam_one(p.x, g.x, m.x, v.x, a);
            adam_one(p.y, g.y, m.y, v.y, a);
            adam_one(p.z, g.z, m.z, v.z, a);
            adam_one(p.w, g.w, m.w, v.w, a);
            *reinterpret_cast<float4*>(t.p + i) = p;
            *reinterpret_cast<float4*>(t.m + i) = m;
            *reinterpret_cast<float4*>(t.v + i) = v;
        } else {
            for (unsigned k = i; k < i + 4 && k < n; ++k) {
                float p = t.p[k], m = t.m[k], v = t.v[k];
                adam_one(p, t.g[k], m, v, a);
                t.p[k] = p; t.m[k] = m; t.v[k] = v;
            }
        }
    }
}

// tensors[count]: p / g / m / v / n filled in by the caller, n >= 1; `first` is assigned here.  As few launches as the
// argument block allows (ADAM_MAX_TENSORS tensors each).
hipError_t launch_adam_multi(AdamTensor* tensors, int count, const AdamScalars& sc, hipStream_t s) {
    for (int i0 = 0; i0 < count; i0 += ADAM_MAX_TENSORS) {
        AdamTable a;
        a.step_size = sc.step_size; a.beta1 = sc.beta1; a.one_minus_beta1 = sc.one_minus_beta1;
        a.beta2 = sc.beta2; a.one_minus_beta2 = sc.one_minus_beta2; a.bc2_sqrt = sc.bc2_sqrt;
        a.eps = sc.eps; a.weight_decay = sc.weight_decay; a.pad = 0;
        a.count = count - i0 < ADAM_MAX_TENSORS ? count - i0 : ADAM_MAX_TENSORS;
        unsigned chunks = 0;
        for (int i = 0; i < a.count; ++i) {
            a.t[i] = tensors[i0 + i];
            a.t[i].first = chunks;
            chunks += (a.t[i].n + ADAM_CHUNK - 1) / ADAM_CHUNK;
        }
        for (int i = a.count; i < ADAM_MAX_TENSORS; ++i) a.t[i] = AdamTensor{nullptr, nullptr, nullptr, nullptr, 0u, 0xffffffffu};
        hipLaunchKernelGGL(adam_multi_kernel, dim3(chunks), dim3(256), 0, s, a);
        const hipError_t rc = hipGetLastError();
        if (rc != hipSuccess) return rc;
    }
    return hipSuccess;
}

// ---- global gradient norm, clip coefficient, clipped / decoupled update -----------------------------------------------
// torch.nn.utils.clip_grad_norm_(parameters, max_norm) (norm_type = 2) without its dozens of small launches and without a
// host read-back: block partials of the squares -> one finishing block -> norm and coefficient as device floats, which the
// update kernel (or grad_scale_multi_kernel) reads.  A block owns ADAM_CHUNK consecutive elements of ONE tensor, as in
// adam_multi_kernel; chunk numbers run on over the launches of one call (NormTable::base), so the partials are one array.
struct NormTable {
    double* partial;                      // [chunks of the whole call]
    const float* coef;                    // grad_scale_multi_kernel only
    unsigned base;                        // global chunk number of this launch's block 0
    int count;
    NormTensor t[ADAM_MAX_TENSORS];
};
static_assert(sizeof(NormTensor) == 16, "a pointer, a length and a first chunk");
static_assert(sizeof(NormTable) <= 4096 - 64, "kernel-argument block limit");

__device__ __forceinline__ int norm_find(const NormTable& a) {
    int lo = 0, hi = a.count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.t[mid].first <= blockIdx.x) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// The squares of fp32 values are exact in double; a thread adds its 8 in a fixed order, the block in block_sum256's tree.
__global__ __launch_bounds__(256) void grad_sumsq_multi_kernel(const NormTable a) {
    __shared__ double red[256];
    const NormTensor t = a.t[norm_find(a)];
    const unsigned off = (blockIdx.x - t.first) * (unsigned)ADAM_CHUNK;
    const unsigned n = t.n;
    const bool vec = (reinterpret_cast<uintptr_t>(t.g) & 15) == 0;
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < ADAM_CHUNK / 1024; ++j) {
        const unsigned i = off + ((unsigned)j * 256 + threadIdx.x) * 4;
        double q[4] = {0.0, 0.0, 0.0, 0.0};
        if (vec && i + 3 < n) {
            const float4 g = *reinterpret_cast<const float4*>(t.g + i);
            q[0] = (double)g.x * (double)g.x; q[1] = (double)g.y * (double)g.y;
            q[2] = (double)g.z * (double)g.z; q[3] = (double)g.w * (double)g.w;
        } else {
            // tail of the tensor, or a pointer that is not 16-byte aligned: the same elements, the same order of additions
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (i + k < n) { const double x = (double)t.g[i + k]; q[k] = x * x; }
        }
        acc += (q[0] + q[1]) + (q[2] + q[3]);
    }
    const double s = block_sum256(acc, red);
    if (threadIdx.x == 0) a.partial[a.base + blockIdx.x] = s;
}

// one block: the partials in ascending order per thread, then the tree (fixed by n_partial alone) -> norm, coefficient.
// coef = min(1, max_norm / (norm + 1e-6)) in fp32 as clip_grad_norm_ forms it (a NaN stays NaN, as torch.clamp keeps it);
// max_norm <= 0: 1.  skip_nonfinite and a norm that is inf or NaN: coef = UPDATE_SKIP_COEF (no clip coefficient is
// negative), which update_multi_kernel and grad_scale_multi_kernel take as "leave everything alone", and *skipped += 1.
constexpr float UPDATE_SKIP_COEF = -1.0f;
__global__ __launch_bounds__(256) void grad_norm_finish_kernel(const double* __restrict__ partial, unsigned n_partial, float max_norm,
                                                               int skip_nonfinite, float* __restrict__ norm_out,
                                                               float* __restrict__ coef_out, unsigned* __restrict__ skipped) {
    __shared__ double red[256];
    double a = 0.0;
    for (unsigned i = threadIdx.x; i < n_partial; i += 256) a += partial[i];
    const double s = block_sum256(a, red);
    if (threadIdx.x != 0) return;
    const float norm = (float)sqrt(s);
    float coef = 1.0f;
    if (max_norm > 0.0f) {
        const float c = max_norm / (norm + 1e-6f);
        coef = c < 1.0f ? c : (c != c ? c : 1.0f);
    }
    if (skip_nonfinite && !(fabsf(norm) <= 3.402823466e+38f)) {
        coef = UPDATE_SKIP_COEF;
        if (skipped) *skipped += 1u;          // one thread of one block, stream-ordered: no atomic needed
    }
    if (norm_out) *norm_out = norm;
    if (coef_out) *coef_out = coef;
}

// g *= coef: the scale pass of lns_amd.optim.clip_grad_norm_ (with the fused step the update kernel scales instead)
__global__ __launch_bounds__(256) void grad_scale_multi_kernel(const NormTable a) {
    const float coef = *a.coef;
    if (coef < 0.0f) return;                  // UPDATE_SKIP_COEF
    const NormTensor t = a.t[norm_find(a)];
    const unsigned off = (blockIdx.x - t.first) * (unsigned)ADAM_CHUNK;
    const unsigned n = t.n;
    float* g = const_cast<float*>(t.g);
    const bool vec = (reinterpret_cast<uintptr_t>(g) & 15) == 0;
#pragma unroll
    for (int j = 0; j < ADAM_CHUNK / 1024; ++j) {
        const unsigned i = off + ((unsigned)j * 256 + threadIdx.x) * 4;
        if (i >= n) break;
        if (vec && i + 3 < n) {
            float4 v = *reinterpret_cast<const float4*>(g + i);
            v.x *= coef; v.y *= coef; v.z *= coef; v.w *= coef;
            *reinterpret_cast<float4*>(g + i) = v;
        } else {
            for (unsigned k = i; k < i + 4 && k < n; ++k) g[k] *= coef;
        }
    }
}

static unsigned norm_fill(NormTable& a, const NormTensor* tensors, int i0, int count) {
    a.count = count - i0 < ADAM_MAX_TENSORS ? count - i0 : ADAM_MAX_TENSORS;
    unsigned chunks = 0;
    for (int i = 0; i < a.count; ++i) {
        a.t[i] = tensors[i0 + i];
        a.t[i].first = chunks;
        chunks += (a.t[i].n + ADAM_CHUNK - 1) / ADAM_CHUNK;
    }
    for (int i = a.count; i < ADAM_MAX_TENSORS; ++i) a.t[i] = NormTensor{nullptr, 0u, 0xffffffffu};
    return chunks;
}

long grad_norm_partials(const NormTensor* tensors, int count) {
    long chunks = 0;
    for (int i = 0; i < count; ++i) chunks += ((long)tensors[i].n + ADAM_CHUNK - 1) / ADAM_CHUNK;
    return chunks;
}

// tensors[count]: g / n filled in by the caller, n >= 1; partial: grad_norm_partials(tensors, count) doubles.
hipError_t launch_grad_norm(const NormTensor* tensors, int count, float max_norm, int skip_nonfinite, float* norm_out, float* coef_out,
                            unsigned* skipped, double* partial, hipStream_t s) {
    unsigned base = 0;
    for (int i0 = 0; i0 < count; i0 += ADAM_MAX_TENSORS) {
        NormTable a;
        a.partial = partial; a.coef = nullptr; a.base = base;
        const unsigned chunks = norm_fill(a, tensors, i0, count);
        hipLaunchKernelGGL(grad_sumsq_multi_kernel, dim3(chunks), dim3(256), 0, s, a);
        const hipError_t rc = hipGetLastError();
        if (rc != hipSuccess) return rc;
        base += chunks;
    }
    hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(256), 0, s, partial, base, max_norm, skip_nonfinite, norm_out, coef_out, skipped);
    return hipGetLastError();
}

hipError_t launch_grad_scale(const NormTensor* tensors, int count, const float* coef, hipStream_t s) {
    for (int i0 = 0; i0 < count; i0 += ADAM_MAX_TENSORS) {
        NormTable a;
        a.partial = nullptr; a.coef = coef; a.base = 0;
        const unsigned chunks = norm_fill(a, tensors, i0, count);
        hipLaunchKernelGGL(grad_scale_multi_kernel, dim3(chunks), dim3(256), 0, s, a);
        const hipError_t rc = hipGetLastError();
        if (rc != hipSuccess) return rc;
    }
    return hipSuccess;
}

// Adam (L2 weight decay, adam_one as it is) or AdamW (decay = 1 - lr weight_decay applied to p first, table.weight_decay = 0)
// on g * coef, which is also what the gradient buffer holds afterwards -- like .grad after clip_grad_norm_.  coef == null:
// the gradient is used and left as it is.
struct UpdateTable {
    const float* coef;
    float decay;                          // decoupled: 1 - lr * weight_decay, rounded once from double; otherwise unused
    int decoupled;
    AdamTable a;
};
static_assert(sizeof(UpdateTable) <= 4096 - 64, "kernel-argument block limit");

// g * coef rounded on its own: the product must be the fp32 value the gradient buffer receives, and must not be contracted
// into adam_one's `g + weight_decay * p` (hipcc contracts by default and honours this pragma) -- with coef == 1 the kernel
// then computes exactly what adam_multi_kernel computes, bit for bit (tests/test_train_clip_gpu.py).
__device__ __forceinline__ float scale_grad(float g, float coef) {
#pragma clang fp contract(off)
    return g * coef;
}

__global__ __launch_bounds__(256) void update_multi_kernel(const UpdateTable u) {
    const float coef = u.coef ? *u.coef : 1.0f;
    if (coef < 0.0f) return;                  // UPDATE_SKIP_COEF: p, exp_avg, exp_avg_sq and the gradient stay
    const bool scale = u.coef != nullptr;
    int lo = 0, hi = u.a.count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (u.a.t[mid].first <= blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const AdamTensor t = u.a.t[lo];
    float* tg = const_cast<float*>(t.g);
    const unsigned off = (blockIdx.x - t.first) * (unsigned)ADAM_CHUNK;
    const unsigned n = t.n;
    const bool vec = ((reinterpret_cast<uintptr_t>(t.p) | reinterpret_cast<uintptr_t>(t.g) | reinterpret_cast<uintptr_t>(t.m) |
                       reinterpret_cast<uintptr_t>(t.v)) & 15) == 0;
#pragma unroll
    for (int j = 0; j < ADAM_CHUNK / 1024; ++j) {
        const unsigned i = off + ((unsigned)j * 256 + threadIdx.x) * 4;
        if (i >= n) break;
        if (vec && i + 3 < n) {
            float4 p = *reinterpret_cast<const float4*>(t.p + i);
            float4 g = *reinterpret_cast<const float4*>(t.g + i);
            float4 m = *reinterpret_cast<const float4*>(t.m + i);
            float4 v = *reinterpret_cast<const float4*>(t.v + i);
            if (scale) {
                g.x = scale_grad(g.x, coef); g.y = scale_grad(g.y, coef); g.z = scale_grad(g.z, coef); g.w = scale_grad(g.w, coef);
                *reinterpret_cast<float4*>(tg + i) = g;
            }
            if (u.decoupled) { p.x *= u.decay; p.y *= u.decay; p.z *= u.decay; p.w *= u.decay; }
            adam_one(p.x, g.x, m.x, v.x, u.a);
            adam_one(p.y, g.y, m.y, v.y, u.a);
            adam_one(p.z, g.z, m.z, v.z, u.a);
            adam_one(p.w, g.w, m.w, v.w, u.a);
            *reinterpret_cast<float4*>(t.p + i) = p;
            *reinterpret_cast<float4*>(t.m + i) = m;
            *reinterpret_cast<float4*>(t.v + i) = v;
        } else {
            for (unsigned k = i; k < i + 4 && k < n; ++k) {
                float p = t.p[k], g = t.g[k], m = t.m[k], v = t.v[k];
                if (scale) { g = scale_grad(g, coef); tg[k] = g; }
                if (u.decoupled) p *= u.decay;
                adam_one(p, g, m, v, u.a);
                t.p[k] = p; t.m[k] = m; t.v[k] = v;
            }
        }
    }
}

// As launch_adam_multi; sc.weight_decay must be 0 when `decoupled` (the caller moves it into `decay`).
hipError_t launch_update_multi(AdamTensor* tensors, int count, const AdamScalars& sc, const float* coef, int decoupled, float decay,
                               hipStream_t s) {
    for (int i0 = 0; i0 < count; i0 += ADAM_MAX_TENSORS) {
        UpdateTable u;
        u.coef = coef; u.decay = decay; u.decoupled = decoupled;
        AdamTable& a = u.a;
        a.step_size = sc.step_size; a.beta1 = sc.beta1; a.one_minus_beta1 = sc.one_minus_beta1;
        a.beta2 = sc.beta2; a.one_minus_beta2 = sc.one_minus_beta2; a.bc2_sqrt = sc.bc2_sqrt;
        a.eps = sc.eps; a.weight_decay = sc.weight_decay; a.pad = 0;
        a.count = count - i0 < ADAM_MAX_TENSORS ? count - i0 : ADAM_MAX_TENSORS;
        unsigned chunks = 0;
        for (int i = 0; i < a.count; ++i) {
            a.t[i] = tensors[i0 + i];
            a.t[i].first = chunks;
            chunks += (a.t[i].n + ADAM_CHUNK - 1) / ADAM_CHUNK;
        }
        for (int i = a.count; i < ADAM_MAX_TENSORS; ++i) a.t[i] = AdamTensor{nullptr, nullptr, nullptr, nullptr, 0u, 0xffffffffu};
        hipLaunchKernelGGL(update_multi_kernel, dim3(chunks), dim3(256), 0, s, u);
        const hipError_t rc = hipGetLastError();
        if (rc != hipSuccess) return rc;
    }
    return hipSuccess;
}

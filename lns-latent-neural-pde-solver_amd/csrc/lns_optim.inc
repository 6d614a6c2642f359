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
// Both are memory-bound elementwise kernels: 16-byte accesses where the pointers allow it, one read of every input.
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

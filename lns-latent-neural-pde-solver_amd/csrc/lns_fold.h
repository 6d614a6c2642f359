// Composition of two adjacent linear convolutions into one set of weights (host only, no HIP: this header also compiles
// into the stand-alone checker tests/native/fold_check.cpp).
//
// A convolution A ([Cmid][Cin][k][k], optional bias) directly followed by a 1x1 convolution B ([Cout][Cmid], optional
// bias) -- nothing in between: no norm, no activation, no residual -- is one convolution with
//     W'[o][i][ky][kx] = sum_m W2[o][m] * W1[m][i][ky][kx]
//     b'[o]            = sum_m W2[o][m] * b1[m] + b2[o]
// exactly, for every padding mode, stride and dilation of A and for A behind a nearest upsample: B acts per output pixel
// of A, and A's bias is added after its padding.  (The other order, a biased 1x1 in FRONT of a zero-padded k x k, is not
// such a map: the padding ring would have to hold W2 b1 instead of 0.)
#pragma once
#include <cstddef>

namespace lns {

// One launch of the composed conv costs k^2 Cin Cout multiply-adds per pixel, the pair k^2 Cin Cmid + Cmid Cout: the fold
// pays when it does not add arithmetic (it always removes a launch, or an epilogue, and the intermediate tensor).
inline bool fold_pays(int k, int cin, int cmid, int cout) {
    const long kk = (long)k * k;
    return kk * cin * cout <= kk * cin * cmid + (long)cmid * cout;
}

namespace fold_detail {
// s + c carries the running sum to about twice double's precision (Neumaier's compensated summation: the two-sum error
// term of every addition is kept in c), so the single rounding to fp32 at the end sees the exact value for all practical
// purposes.  Every product of two fp32 values is exact in double.
struct Acc {
    double s = 0.0, c = 0.0;
    void add(double v) {
        const double t = s + v;
        const double as = s < 0 ? -s : s, av = v < 0 ? -v : v;
        c += as >= av ? (s - t) + v : (v - t) + s;
        s = t;
    }
    float value() const { return (float)(s + c); }
};
}  // namespace fold_detail

// w1 [cmid][cin][k][k], b1 [cmid] or nullptr; w2 [cout][cmid] (a 1x1 conv's [cout][cmid][1][1]), b2 [cout] or nullptr.
// Writes w_out [cout][cin][k][k] and, when either bias exists, b_out [cout]; returns whether the composed conv has a bias.
// Accumulates in double, rounds to fp32 once.
inline bool fold_conv_1x1(const float* w1, const float* b1, const float* w2, const float* b2, int k, int cin, int cmid,
                          int cout, float* w_out, float* b_out) {
    const size_t per_m = (size_t)cin * k * k;      // elements of one mid channel's filter bank = of one output channel's
    for (int o = 0; o < cout; ++o) {
        const float* r2 = w2 + (size_t)o * cmid;
        for (size_t j = 0; j < per_m; ++j) {
            fold_detail::Acc a;
            for (int m = 0; m < cmid; ++m) a.add((double)r2[m] * (double)w1[(size_t)m * per_m + j]);
            w_out[(size_t)o * per_m + j] = a.value();
        }
    }
    const bool has_bias = b1 != nullptr || b2 != nullptr;
    if (has_bias)
        for (int o = 0; o < cout; ++o) {
            fold_detail::Acc a;
            if (b1) for (int m = 0; m < cmid; ++m) a.add((double)w2[(size_t)o * cmid + m] * (double)b1[m]);
            if (b2) a.add((double)b2[o]);
            b_out[o] = a.value();
        }
    return has_bias;
}

}  // namespace lns

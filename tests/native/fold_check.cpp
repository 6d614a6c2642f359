// Stand-alone checker of csrc/lns_fold.h (tests/test_fold_cpu.py builds it with the host compiler and
// -fsanitize=address,undefined and runs it directly).
//
// fold_conv_1x1 against a plain loop nest in long double: the fp32 result must equal the long double result rounded to
// fp32, element for element, on ragged shapes and with every combination of biases; fold_pays on the two sites of the
// square autoencoder and on a shape where it must say no.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "lns_fold.h"

namespace {

// deterministic values in (-1, 1) with a wide spread of magnitudes (so that sums cancel and rounding matters)
struct Rng {
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 0x1234567ull) {}
    uint64_t next() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
    float value() {
        const uint64_t r = next();
        const float m = (float)((r >> 11) & 0xFFFFFF) / 8388608.0f - 1.0f;     // 24 random bits -> [-1, 1)
        const int e = (int)((r >> 40) % 12);                                      // scaled by 2^-e, e in 0..11
        return m / (float)(1 << e);
    }
};

void fill(std::vector<float>& v, Rng& r) { for (float& x : v) x = r.value(); }

int check_shape(int k, int cin, int cmid, int cout, bool bias_a, bool bias_b, uint64_t seed) {
    Rng rng(seed);
    const size_t per = (size_t)cin * k * k;
    std::vector<float> w1((size_t)cmid * per), b1((size_t)cmid), w2((size_t)cout * cmid), b2((size_t)cout);
    fill(w1, rng); fill(b1, rng); fill(w2, rng); fill(b2, rng);
    // exact-size outputs (the sanitizer sees any write past them); the bias array holds a sentinel
    std::vector<float> w((size_t)cout * per, 123.0f), b((size_t)cout, 123.0f);
    const bool has_bias = lns::fold_conv_1x1(w1.data(), bias_a ? b1.data() : nullptr, w2.data(), bias_b ? b2.data() : nullptr, k,
                                            cin, cmid, cout, w.data(), b.data());
    int bad = 0;
    if (has_bias != (bias_a || bias_b)) { printf("  has_bias = %d, expected %d\n", (int)has_bias, (int)(bias_a || bias_b)); ++bad; }
    for (int o = 0; o < cout; ++o)
        for (int i = 0; i < cin; ++i)
            for (int ky = 0; ky < k; ++ky)
                for (int kx = 0; kx < k; ++kx) {
                    long double acc = 0.0L;
                    for (int m = 0; m < cmid; ++m)
                        acc += (long double)w2[(size_t)o * cmid + m] * (long double)w1[(((size_t)m * cin + i) * k + ky) * k + kx];
                    const float want = (float)acc;
                    const float got = w[(((size_t)o * cin + i) * k + ky) * k + kx];
                    if (memcmp(&want, &got, 4) != 0 && bad++ < 8)
                        printf("  W'[%d][%d][%d][%d] = %.9g, long double gives %.9g\n", o, i, ky, kx, (double)got, (double)want);
                }
    for (int o = 0; o < cout; ++o) {
        float want = 123.0f;                                  // no bias on either side: b_out is left alone
        if (bias_a || bias_b) {
            long double acc = 0.0L;
            if (bias_a) for (int m = 0; m < cmid; ++m) acc += (long double)w2[(size_t)o * cmid + m] * (long double)b1[m];
            if (bias_b) acc += (long double)b2[o];
            want = (float)acc;
        }
        if (memcmp(&want, &b[o], 4) != 0 && bad++ < 8) printf("  b'[%d] = %.9g, long double gives %.9g\n", o, (double)b[o], (double)want);
    }
    printf("fold k=%d %d->%d->%d bias_a=%d bias_b=%d: %s\n", k, cin, cmid, cout, (int)bias_a, (int)bias_b, bad ? "MISMATCH" : "ok");
    return bad;
}

}  // namespace

int main() {
    const int shapes[3][4] = {{3, 5, 7, 3}, {1, 16, 16, 128}, {3, 64, 64, 64}};    // k, Cin, Cmid, Cout
    int bad = 0;
    uint64_t seed = 1;
    for (const auto& s : shapes)
        for (int ba = 0; ba < 2; ++ba)
            for (int bb = 0; bb < 2; ++bb) bad += check_shape(s[0], s[1], s[2], s[3], ba != 0, bb != 0, seed++);
    struct { int k, cin, cmid, cout; bool want; const char* what; } rules[] = {
        {3, 64, 64, 64, true, "decoder tail 3x3 -> 1x1"},
        {1, 16, 16, 128, true, "post_quant_conv -> decoder.model.0"},
        {1, 128, 16, 16, true, "encoder's last 1x1 -> quant_conv"},
        {1, 16, 128, 128, true, "1x1 16 -> 128 -> 128 (2048 <= 2048 + 16384)"},
        {1, 128, 16, 128, false, "1x1 through a 16-channel bottleneck, 128 -> 16 -> 128 (the fold would add arithmetic)"},
        {3, 8, 4, 64, false, "3x3 through a 4-channel bottleneck"},
    };
    for (const auto& r : rules) {
        const bool got = lns::fold_pays(r.k, r.cin, r.cmid, r.cout);
        printf("fold_pays %s: %d (expected %d)\n", r.what, (int)got, (int)r.want);
        if (got != r.want) ++bad;
    }
    printf(bad ? "FAILED\n" : "ALL OK\n");
    return bad ? 1 : 0;
}

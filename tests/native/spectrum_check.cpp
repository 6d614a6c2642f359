// Stand-alone check of csrc/lns_spectrum.h (host only; built with -fsanitize=address,undefined by tests/test_eval_spectrum_cpu.py):
// the shell rule against a brute-force search, the bin count, the support rule, the conjugate weights, the run structure
// the kernel's shell walk relies on (along a row the shell does not decrease with kx and rises by at most one per column,
// every bin has a mode) and the LDS layout, for every supported (H, W) with H, W <= 64 and the presets' planes.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lns_spectrum.h"

using namespace lns_spectrum;

static int brute_shell(int r2) {
    for (int s = 0;; ++s)
        if ((s == 0 ? r2 == 0 : (long)s * (s - 1) < r2) && r2 <= (long)s * (s + 1)) return s;
}

static int fails = 0;
#define CHECK(cond, ...)                                                    \
    do {                                                                    \
        if (!(cond)) { printf("FAIL: " __VA_ARGS__); printf("\n"); ++fails; } \
    } while (0)

static void check_plane(int H, int W) {
    CHECK(supported(H, W), "%dx%d should be supported", H, W);
    const int S = bins(H, W), Wh = W / 2 + 1;
    CHECK(S == brute_shell((H / 2) * (H / 2) + (W / 2) * (W / 2)) + 1, "bins %dx%d = %d", H, W, S);
    CHECK(S >= 1 && S <= 256, "bins %dx%d = %d does not fit a block's threads", H, W, S);
    std::vector<int> seen(S, 0);
    for (int ky = 0; ky < H; ++ky) {
        const int q = signed_k(ky, H);
        CHECK(q == (ky <= H / 2 ? ky : ky - H) && q > -H && q <= H / 2, "signed_k(%d, %d) = %d", ky, H, q);
        int prev = -1;
        for (int kx0 = 0; kx0 < Wh; kx0 += KX_TILE) {
            int runs = 0;
            for (int kx = kx0; kx < Wh && kx < kx0 + KX_TILE; ++kx) {
                const int s = mode_shell(ky, kx, H);
                CHECK(s == brute_shell(q * q + kx * kx), "mode_shell(%d, %d, %d) = %d", ky, kx, H, s);
                CHECK(s >= 0 && s < S, "mode (%d, %d) of %dx%d has shell %d outside [0, %d)", ky, kx, H, W, s, S);
                CHECK(kx == 0 || (s >= prev && s <= prev + 1), "row %d of %dx%d: shell goes %d -> %d at kx %d", ky, H, W, prev, s, kx);
                if (kx == kx0 || s != prev) ++runs;
                prev = s;
                if (s >= 0 && s < S) seen[s] = 1;
            }
            CHECK(runs <= KX_TILE, "row %d of %dx%d: %d runs in a tile", ky, H, W, runs);
        }
    }
    for (int s = 0; s < S; ++s) CHECK(seen[s], "bin %d of %dx%d has no mode", s, H, W);
    for (int kx = 0; kx < Wh; ++kx)
        CHECK(weight(kx, W) == ((kx == 0 || 2 * kx == W) ? 1 : 2), "weight(%d, %d) = %d", kx, W, weight(kx, W));
    const Lds l = lds_layout(H, W);
    const int expect = H * (W | 1) + 3 * H * PITCH + 2 * W + 4 * H;
    CHECK(l.total == expect && l.field == 0 && l.re == H * (W | 1) && l.im == l.re + H * PITCH && l.pw == l.im + H * PITCH &&
              l.cw == l.pw + H * PITCH && l.sw == l.cw + W && l.ch == l.sw + W && l.sh == l.ch + H && l.s0 == l.sh + H &&
              l.n == l.s0 + H && l.total == l.n + H,
          "lds_layout %dx%d", H, W);
    CHECK(lds_bytes(H, W) == 4L * expect && lds_bytes(H, W) <= 160 * 1024, "lds_bytes %dx%d = %ld", H, W, lds_bytes(H, W));
}

int main() {
    for (int r2 = 0; r2 <= 2 * 192 * 192; ++r2) CHECK(shell(r2) == brute_shell(r2), "shell(%d) = %d", r2, shell(r2));
    printf("shell rule 0 .. %d: %s\n", 2 * 192 * 192, fails ? "FAILED" : "ok");
    CHECK(shell(-1) == 0, "shell(-1)");
    // the kernel's run walk: along a row the shell never decreases and rises by at most one per column.  The property depends
    // on (|ky'|, kx) only, so this covers every supported plane (|ky'| <= 96, kx <= 96), and more
    for (int q = 0; q <= MAX_DIM; ++q)
        for (int kx = 0; kx < MAX_DIM; ++kx) {
            const int d = shell(q * q + (kx + 1) * (kx + 1)) - shell(q * q + kx * kx);
            CHECK(d == 0 || d == 1, "shell step %d at |ky'| = %d, kx = %d -> %d", d, q, kx, kx + 1);
        }
    printf("run walk 0 .. %d: %s\n", MAX_DIM, fails ? "FAILED" : "ok");
    int planes = 0;
    for (int H = 1; H <= 64; ++H)
        for (int W = 1; W <= 64; ++W) { check_plane(H, W); ++planes; }
    const int presets[][2] = {{32, 32}, {64, 64}, {128, 128}, {96, 192}, {192, 96}, {61, 121}, {121, 61}, {1, 192}, {192, 1}, {135, 136}};
    for (const auto& p : presets) { check_plane(p[0], p[1]); ++planes; }
    printf("planes checked: %d\n", planes);
    const int known[][3] = {{32, 32, 24}, {128, 128, 92}, {96, 192, 108}, {61, 121, 68}};
    for (const auto& k : known) {
        CHECK(bins(k[0], k[1]) == k[2], "bins(%d, %d) = %d, expected %d", k[0], k[1], bins(k[0], k[1]), k[2]);
        printf("bins %dx%d: %d\n", k[0], k[1], bins(k[0], k[1]));
    }
    const int refused[][2] = {{129, 144}, {1, 193}, {193, 1}, {0, 5}, {5, 0}, {-3, 4}, {192, 97}};
    for (const auto& r : refused) CHECK(!supported(r[0], r[1]) && bins(r[0], r[1]) == -1, "%dx%d should be refused", r[0], r[1]);
    // the largest LDS request over every supported plane stays inside the 160 KB of a compute unit
    long worst = 0;
    for (int H = 1; H <= MAX_DIM; ++H)
        for (int W = 1; W <= MAX_DIM; ++W)
            if (supported(H, W)) {
                if (lds_bytes(H, W) > worst) worst = lds_bytes(H, W);
                CHECK(bins(H, W) <= 256, "bins(%d, %d)", H, W);
            }
    CHECK(worst <= 160 * 1024, "largest LDS request %ld", worst);
    printf("largest LDS request: %ld bytes\n", worst);
    if (fails) { printf("%d FAILURES\n", fails); return 1; }
    printf("ALL OK\n");
    return 0;
}

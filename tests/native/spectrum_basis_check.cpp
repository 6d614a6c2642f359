// Stand-alone check of the basis-aware half of csrc/lns_spectrum.h (host only; built with -fsanitize=address,undefined by
// tests/test_spectrum_basis_cpu.py): the half-unit shell map and the bin count against brute force, the weights, the run
// structure the kernel's shell walk relies on (along a row the shell does not decrease and rises by at most the column's
// step in half units -- two for a DFT x axis, one for a DCT one -- so a tile's run sums fit their row), every bin below
// S <= 256, and the LDS layout, for every supported (H, W) with H, W <= 64 and the presets' planes, under all four bases.
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

static int widest = 0;   // the widest span of shells of one row in one tile, DCT y with DFT x

static void check_plane(int H, int W, int by, int bx) {
    const int S = bins(H, W, by, bx), NX = columns(W, bx);
    if (by == DFT && bx == DFT) {
        CHECK(S == bins(H, W), "bins %dx%d dft/dft = %d", H, W, S);
        const Lds a = lds_layout(H, W), b = lds_layout(H, W, by, bx);
        CHECK(a.total == b.total && a.s0 == b.s0 && a.n == b.n && a.sh == b.sh, "lds_layout %dx%d dft/dft differs", H, W);
        return;
    }
    CHECK(NX == (bx == DCT ? W : W / 2 + 1), "columns(%d, %d) = %d", W, bx, NX);
    int top = 0;
    for (int ky = 0; ky < H; ++ky)
        for (int kx = 0; kx < NX; ++kx) {
            const int qy = by == DCT ? ky : 2 * (ky <= H / 2 ? ky : ky - H), qx = bx == DCT ? kx : 2 * kx;
            const int s = brute_shell(qy * qy + qx * qx);
            CHECK(half_y(ky, H, by) == qy && half_x(kx, bx) == qx, "half counts of (%d, %d) in %dx%d basis %d%d", ky, kx, H, W, by, bx);
            CHECK(mode_shell_half(ky, kx, H, by, bx) == s, "mode_shell_half(%d, %d) of %dx%d basis %d%d", ky, kx, H, W, by, bx);
            if (s > top) top = s;
        }
    CHECK(S == top + 1, "bins %dx%d basis %d%d = %d, brute force %d", H, W, by, bx, S, top + 1);
    CHECK(S >= 1 && S <= 256, "bins %dx%d basis %d%d = %d does not fit a block's threads", H, W, by, bx, S);
    const int rise = bx == DCT ? 1 : 2, room = (by == DCT && bx == DFT) ? (int)RUNS_WIDE : (int)PITCH;
    for (int ky = 0; ky < H; ++ky) {
        int prev = -1;
        for (int kx0 = 0; kx0 < NX; kx0 += KX_TILE) {
            const int first = mode_shell_half(ky, kx0, H, by, bx);
            for (int kx = kx0; kx < NX && kx < kx0 + KX_TILE; ++kx) {
                const int s = mode_shell_half(ky, kx, H, by, bx);
                CHECK(kx == 0 || (s >= prev && s <= prev + rise), "row %d of %dx%d basis %d%d: shell goes %d -> %d at kx %d", ky, H, W, by, bx, prev, s, kx);
                CHECK(s - first >= 0 && s - first < room, "row %d of %dx%d basis %d%d: run %d of a tile", ky, H, W, by, bx, s - first);
                if (by == DCT && bx == DFT && s - first + 1 > widest) widest = s - first + 1;
                prev = s;
            }
        }
    }
    for (int k = 0; k < H; ++k) CHECK(weight_y(k, by) == (by == DCT ? (k == 0 ? 1 : 2) : 1), "weight_y(%d, %d)", k, by);
    for (int k = 0; k < NX; ++k)
        CHECK(weight_x(k, W, bx) == (bx == DCT ? (k == 0 ? 1 : 2) : weight(k, W)), "weight_x(%d, %d, %d)", k, W, bx);
    const Lds l = lds_layout(H, W, by, bx);
    const int im = bx == DCT ? 0 : H * PITCH, tx = bx == DCT ? 4 * W : 2 * W, ty = by == DCT ? 4 * H : 2 * H;
    CHECK(l.field == 0 && l.re == H * (W | 1) && l.im == l.re + H * PITCH && l.pw == l.im + im && l.cw == l.pw + H * PITCH &&
              l.ch == l.cw + tx && l.s0 == l.ch + ty && l.n == l.s0 + H && l.total == l.n + H,
          "lds_layout %dx%d basis %d%d", H, W, by, bx);
    CHECK(bx == DCT || l.sw == l.cw + W, "sw of %dx%d basis %d%d", H, W, by, bx);
    CHECK(by == DCT || l.sh == l.ch + H, "sh of %dx%d basis %d%d", H, W, by, bx);
    // the wide run rows live in re | im, which are contiguous
    CHECK(!(by == DCT && bx == DFT) || (l.pw - l.re == H * RUNS_WIDE), "run rows of %dx%d", H, W);
    CHECK(lds_bytes(H, W, by, bx) == 4L * l.total && lds_bytes(H, W, by, bx) <= 160 * 1024, "lds_bytes %dx%d basis %d%d = %ld", H, W,
          by, bx, lds_bytes(H, W, by, bx));
}

int main() {
    int planes = 0;
    for (int by = 0; by < 2; ++by)
        for (int bx = 0; bx < 2; ++bx) {
            for (int H = 1; H <= 64; ++H)
                for (int W = 1; W <= 64; ++W) { check_plane(H, W, by, bx); ++planes; }
            const int presets[][2] = {{32, 32}, {64, 64}, {128, 128}, {96, 192}, {192, 96}, {61, 121}, {121, 61}, {1, 192}, {192, 1}, {135, 136}, {24, 48}};
            for (const auto& p : presets) { check_plane(p[0], p[1], by, bx); ++planes; }
        }
    printf("planes x bases checked: %d\n", planes);
    printf("widest run row (dct y, dft x): %d of %d\n", widest, (int)RUNS_WIDE);
    const int known[][5] = {{24, 48, 54, 54, 53}, {61, 121, 135, 135, 135}, {96, 192, 215, 215, 214}, {128, 128, 181, 181, 181}};
    for (const auto& k : known) {
        const int a = bins(k[0], k[1], DCT, DFT), b = bins(k[0], k[1], DFT, DCT), c = bins(k[0], k[1], DCT, DCT);
        CHECK(a == k[2] && b == k[3] && c == k[4], "bins of %dx%d: %d / %d / %d", k[0], k[1], a, b, c);
        printf("bins %dx%d: %d / %d / %d\n", k[0], k[1], a, b, c);
    }
    const int refused[][4] = {{129, 144, 1, 1}, {1, 193, 1, 0}, {0, 5, 0, 1}, {32, 32, 2, 0}, {32, 32, 0, -1}, {32, 32, 1, 2}};
    for (const auto& r : refused) CHECK(bins(r[0], r[1], r[2], r[3]) == -1, "%dx%d basis %d %d should be refused", r[0], r[1], r[2], r[3]);
    // over every supported plane: the largest S fits a block's threads, the largest LDS request the 160 KB of a compute unit
    long worst = 0;
    int top = 0;
    for (int by = 0; by < 2; ++by)
        for (int bx = 0; bx < 2; ++bx)
            for (int H = 1; H <= MAX_DIM; ++H)
                for (int W = 1; W <= MAX_DIM; ++W)
                    if (supported(H, W)) {
                        if (lds_bytes(H, W, by, bx) > worst) worst = lds_bytes(H, W, by, bx);
                        if (bins(H, W, by, bx) > top) top = bins(H, W, by, bx);
                    }
    CHECK(top <= 256, "largest S %d", top);
    CHECK(worst <= 160 * 1024, "largest LDS request %ld", worst);
    printf("largest S: %d\n", top);
    printf("largest LDS request: %ld bytes\n", worst);
    if (fails) { printf("%d FAILURES\n", fails); return 1; }
    printf("ALL OK\n");
    return 0;
}

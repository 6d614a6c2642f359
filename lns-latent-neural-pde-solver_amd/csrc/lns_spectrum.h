// Shell-summed energy spectrum (include/lns.h "energy spectra"): the integer side of the statement, with no HIP in it.
// Shared by the library (host checks, launch sizes, and the kernel's own shell walk) and by tests/native/spectrum_check.cpp.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LNS_SPEC_HD __host__ __device__
#else
#define LNS_SPEC_HD
#endif

namespace lns_spectrum {

enum { MAX_DIM = 192, MAX_PIXELS = 18432, KX_TILE = 32, PITCH = KX_TILE + 1 };

// the integer s with s (s - 1) < r2 <= s (s + 1); 0 for r2 = 0: round(sqrt(r2)) with no floating tie.
// A binary search for the largest s with s (s - 1) < r2 (then r2 <= s (s + 1), or s + 1 would qualify too): exact for
// every r2 whose s (s + 1) fits an int; r2 <= 2 * 192^2 here.
LNS_SPEC_HD inline int shell(int r2) {
    if (r2 <= 0) return 0;
    int bit = 1;                                   // the largest power of two with bit (bit - 1) < r2
    while (bit < 32768 && (2 * bit) * (2 * bit - 1) < r2) bit *= 2;
    int s = bit;
    for (bit /= 2; bit > 0; bit /= 2)
        if ((s + bit) * (s + bit - 1) < r2) s += bit;
    return s;
}

// signed wavenumber of row ky
LNS_SPEC_HD inline int signed_k(int k, int N) { return k <= N / 2 ? k : k - N; }

// shell of mode (ky, kx) of an H x W plane, kx in [0, W / 2]
LNS_SPEC_HD inline int mode_shell(int ky, int kx, int H) {
    const int q = signed_k(ky, H);
    return shell(q * q + kx * kx);
}

inline bool supported(int H, int W) {
    return H >= 1 && W >= 1 && H <= MAX_DIM && W <= MAX_DIM && (long)H * W <= MAX_PIXELS;
}

// number of bins S(H, W), or -1 for an unsupported plane
inline int bins(int H, int W) {
    if (!supported(H, W)) return -1;
    return shell((H / 2) * (H / 2) + (W / 2) * (W / 2)) + 1;
}

// conjugate weight of column kx: 1 for kx = 0 and for the Nyquist column of an even W, else 2
LNS_SPEC_HD inline int weight(int kx, int W) { return (kx == 0 || (W % 2 == 0 && kx == W / 2)) ? 1 : 2; }

// The kernel's dynamic LDS, in floats (every region a whole number of floats; the two int arrays are counted as floats):
//   field [H][W | 1]  |  re, im [H][PITCH] each  |  power / run sums [H][PITCH]  |  cos, -sin of both axes  |  s0, n [H] each
struct Lds { int field, re, im, pw, cw, sw, ch, sh, s0, n, total; };
LNS_SPEC_HD inline Lds lds_layout(int H, int W) {
    Lds l;
    int o = 0;
    l.field = o; o += H * (W | 1);
    l.re = o; o += H * PITCH;
    l.im = o; o += H * PITCH;
    l.pw = o; o += H * PITCH;
    l.cw = o; o += W;
    l.sw = o; o += W;
    l.ch = o; o += H;
    l.sh = o; o += H;
    l.s0 = o; o += H;
    l.n = o; o += H;
    l.total = o;
    return l;
}
inline long lds_bytes(int H, int W) { return 4L * lds_layout(H, W).total; }

// ---- a basis per axis (include/lns.h "energy spectra", the wall-aware form): DFT = 0 as above, DCT = 1 (DCT-II) -------
// With a DCT axis, wavenumbers count HALF cycles per side: a DCT index m counts m, a DFT wavenumber k counts 2 k, so
// bin s of such a spectrum lies at s / 2 cycles per side.  Both axes DFT: everything above, unchanged.
enum { DFT = 0, DCT = 1 };

inline bool basis_ok(int by, int bx) { return (by == DFT || by == DCT) && (bx == DFT || bx == DCT); }

// columns a basis stores along x: W / 2 + 1 conjugate-weighted ones (DFT) or all W (DCT)
LNS_SPEC_HD inline int columns(int W, int bx) { return bx == DCT ? W : W / 2 + 1; }

// half-cycle count of row ky / column kx
LNS_SPEC_HD inline int half_y(int ky, int H, int by) { return by == DCT ? ky : 2 * signed_k(ky, H); }
LNS_SPEC_HD inline int half_x(int kx, int bx) { return bx == DCT ? kx : 2 * kx; }

// shell of mode (ky, kx) in half units (not for DFT / DFT: mode_shell)
LNS_SPEC_HD inline int mode_shell_half(int ky, int kx, int H, int by, int bx) {
    const int qy = half_y(ky, H, by), qx = half_x(kx, bx);
    return shell(qy * qy + qx * qx);
}

// weight of row ky / column kx: a DCT index is 1 at 0, else 2 (no Nyquist exception); a DFT row has no partner to stand for
LNS_SPEC_HD inline int weight_y(int ky, int by) { return by == DCT ? (ky == 0 ? 1 : 2) : 1; }
LNS_SPEC_HD inline int weight_x(int kx, int W, int bx) { return bx == DCT ? (kx == 0 ? 1 : 2) : weight(kx, W); }

// number of bins S(H, W, basis), or -1 for an unsupported plane or basis
inline int bins(int H, int W, int by, int bx) {
    if (!supported(H, W) || !basis_ok(by, bx)) return -1;
    if (by == DFT && bx == DFT) return bins(H, W);
    const int qy = by == DCT ? H - 1 : 2 * (H / 2), qx = bx == DCT ? W - 1 : 2 * (W / 2);
    return shell(qy * qy + qx * qx) + 1;
}

// The LDS of a plane with at least one DCT axis.  A DCT axis of length N holds one table of 4 N floats (cw / ch) in place
// of the DFT's two of N; a DCT x axis has no imaginary row-pass part (im, sw unused and not laid out).  DCT y with DFT x:
// along a row the half-unit shell can rise by two per column, so the run sums of a 32-column tile span up to RUNS_WIDE
// shells; they are kept in re | im (contiguous, [H][RUNS_WIDE]) once the column pass has read them.
enum { RUNS_WIDE = 2 * PITCH };
LNS_SPEC_HD inline Lds lds_layout(int H, int W, int by, int bx) {
    if (by == DFT && bx == DFT) return lds_layout(H, W);
    Lds l;
    int o = 0;
    l.field = o; o += H * (W | 1);
    l.re = o; o += H * PITCH;
    l.im = o; o += bx == DCT ? 0 : H * PITCH;
    l.pw = o; o += H * PITCH;
    l.cw = o; o += bx == DCT ? 4 * W : W;
    l.sw = o; o += bx == DCT ? 0 : W;
    l.ch = o; o += by == DCT ? 4 * H : H;
    l.sh = o; o += by == DCT ? 0 : H;
    l.s0 = o; o += H;
    l.n = o; o += H;
    l.total = o;
    return l;
}
inline long lds_bytes(int H, int W, int by, int bx) { return 4L * lds_layout(H, W, by, bx).total; }

}  // namespace lns_spectrum

// ---- shell-summed energy spectra (lns_kernels.h SpectrumArgs; the statement: include/lns.h "energy spectra") ---------
// One block of four waves owns one plane (b, step, c) and writes its K x S floats itself.  The 2-D DFT of a field is two
// dense contractions on the fp32 matrix pipe (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain, bit for bit), tiled over
// kx in tiles of KX_TILE = 32 columns so that both intermediates of a tile fit LDS beside the staged field:
//   stage     the field (forecast P, truth Q, error P - Q, in this order; D_c applied on the way) from global to LDS,
//             rows padded to an odd pitch: the A operand reads 32 rows at one x, which an even pitch puts in one bank
//   row pass  R[y][kx] = sum_x u[y][x] (cos, -sin)(2 pi kx x / W): A = field rows, B = the table at (kx x) mod W
//   col pass  F[ky][kx] = sum_y cos . R  then  sum_y (-/+ sin) . R, one chain per part (order in include/lns.h)
//   power     p = w (a a + b b), a = re inv, b = im inv, into pw[ky][kx - kx0]
//   shells    thread ky folds its row's runs of equal shell (ascending kx) in place and records first shell / run count;
//             thread s then adds the runs of shell s in ascending ky to its running E[s] (ascending tiles)
// Tile edges are zero-padded on BOTH operands of the summed index (0 x 0: a NaN pixel cannot leak through a padded k);
// rows / columns past H / Wh of a result tile are computed and dropped.  All LDS is dynamic (lns_spectrum::lds_layout).
// spectrum_plane is the DFT / DFT body and stays as it is (its bits are the library's record); a plane with a DCT axis goes
// through spectrum_plane_basis below, and the two kernels choose by SpectrumArgs::basis.
namespace lsp = lns_spectrum;

__device__ __forceinline__ void spectrum_plane(const float* f, const float* g, float* out, int H, int W, int S, float sd,
                                               float mean, bool walls, bool clampv, float lo, float hi, float* sm) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, kh = lane >> 5;
    const int HW = H * W, Wh = W / 2 + 1, xp = W | 1;
    const lsp::Lds L = lsp::lds_layout(H, W);
    float *X = sm + L.field, *Rre = sm + L.re, *Rim = sm + L.im, *Pw = sm + L.pw;
    float *cw = sm + L.cw, *sw = sm + L.sw, *ch = sm + L.ch, *sh = sm + L.sh;
    int *s0 = reinterpret_cast<int*>(sm + L.s0), *nr = reinterpret_cast<int*>(sm + L.n);
    for (int r = tid; r < W; r += 256) { float s, c; sincospif(2.0f * (float)r / (float)W, &s, &c); cw[r] = c; sw[r] = -s; }
    for (int r = tid; r < H; r += 256) { float s, c; sincospif(2.0f * (float)r / (float)H, &s, &c); ch[r] = c; sh[r] = -s; }
    const float inv = 1.0f / (float)HW;
    const int nf = g ? 3 : 1;
    for (int fi = 0; fi < nf; ++fi) {
        // eight pixels per thread and trip: the global loads of a trip are issued together (one load's latency per trip, not per pixel)
        for (int i0 = tid; i0 < HW; i0 += 256 * 8) {
            float fv[8], gv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = min(i0 + u * 256, HW - 1);
                fv[u] = fi != 1 ? f[i] : 0.0f;
                gv[u] = fi != 0 ? g[i] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = i0 + u * 256;
                if (i < HW) {
                    const int r = i / W, cx = i - r * W;
                    const bool zero = walls && (r == 0 || r == H - 1 || cx == 0 || cx == W - 1);
                    float v;
                    if (fi == 0) v = score_denorm(fv[u], sd, mean, zero, clampv, lo, hi);
                    else {
                        const float q = score_denorm(gv[u], sd, mean, zero, clampv, lo, hi);
                        v = fi == 1 ? q : score_denorm(fv[u], sd, mean, zero, clampv, lo, hi) - q;
                    }
                    X[r * xp + cx] = v;
                }
            }
        }
        __syncthreads();
        float E = 0.0f;
        for (int kx0 = 0; kx0 < Wh; kx0 += lsp::KX_TILE) {
            // row pass: R[y][kx0 + 0 .. 31], x ascending in one chain per part
            for (int mt = wave; mt * 32 < H; mt += 4) {
                f32x16 are, aim;
#pragma unroll
                for (int r = 0; r < 16; ++r) { are[r] = 0.0f; aim[r] = 0.0f; }
                const int y = mt * 32 + l31;
                const bool yok = y < H;
                const float* xr = X + (yok ? y : 0) * xp;
                const int kx = kx0 + l31;
                int idx = (kx * kh) % W;
                const int step = (2 * kx) % W;
                for (int x0 = 0; x0 < W; x0 += 2) {
                    const int x = x0 + kh;
                    const bool xok = x < W;
                    float av = xr[xok ? x : 0], bc = cw[idx], bs = sw[idx];
                    av = (yok && xok) ? av : 0.0f; bc = xok ? bc : 0.0f; bs = xok ? bs : 0.0f;
                    are = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bc, are, 0, 0, 0);
                    aim = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bs, aim, 0, 0, 0);
                    idx += step; if (idx >= W) idx -= W;
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int yy = mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                    if (yy < H) { Rre[yy * lsp::PITCH + l31] = are[r]; Rim[yy * lsp::PITCH + l31] = aim[r]; }
                }
            }
            __syncthreads();
            // column pass: with e^{-i t} = c + i m (m = -sin t), re = sum c Rre + sum (-m) Rim, im = sum c Rim + sum m Rre
            for (int mt = wave; mt * 32 < H; mt += 4) {
                f32x16 fre, fim;
#pragma unroll
                for (int r = 0; r < 16; ++r) { fre[r] = 0.0f; fim[r] = 0.0f; }
                const int ky = mt * 32 + l31;
                const int step = (2 * ky) % H;
                int idx = (ky * kh) % H;
                for (int y0 = 0; y0 < H; y0 += 2) {
                    const int y = y0 + kh;
                    const bool ok = y < H;
                    const int ro = (ok ? y : 0) * lsp::PITCH + l31;
                    float ac = ch[idx], br = Rre[ro], bi = Rim[ro];
                    ac = ok ? ac : 0.0f; br = ok ? br : 0.0f; bi = ok ? bi : 0.0f;
                    fre = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, br, fre, 0, 0, 0);
                    fim = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, bi, fim, 0, 0, 0);
                    idx += step; if (idx >= H) idx -= H;
                }
                idx = (ky * kh) % H;
                for (int y0 = 0; y0 < H; y0 += 2) {
                    const int y = y0 + kh;
                    const bool ok = y < H;
                    const int ro = (ok ? y : 0) * lsp::PITCH + l31;
                    float am = sh[idx], br = Rre[ro], bi = Rim[ro];
                    am = ok ? am : 0.0f; br = ok ? br : 0.0f; bi = ok ? bi : 0.0f;
                    fre = __builtin_amdgcn_mfma_f32_32x32x2f32(-am, bi, fre, 0, 0, 0);
                    fim = __builtin_amdgcn_mfma_f32_32x32x2f32(am, br, fim, 0, 0, 0);
                    idx += step; if (idx >= H) idx -= H;
                }
                const int kxx = kx0 + l31;
                const float wgt = (float)lsp::weight(kxx, W);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int kyy = mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                    float p = 0.0f;
                    if (kxx < Wh) {
                        const float a = fre[r] * inv, b = fim[r] * inv;
                        const float aa = a * a, bb = b * b;
                        p = wgt * (aa + bb);
                    }
                    if (kyy < H) Pw[kyy * lsp::PITCH + l31] = p;
                }
            }
            __syncthreads();
            // runs of equal shell along row ky, ascending kx, folded in place (run i closes after element i was read)
            if (tid < H) {
                const int q = lsp::signed_k(tid, H), q2 = q * q;
                const int cnt = min(lsp::KX_TILE, Wh - kx0);
                float* row = Pw + tid * lsp::PITCH;
                int s = lsp::shell(q2 + kx0 * kx0), nrun = 0;
                float run = 0.0f;
                s0[tid] = s;
                float pv[lsp::KX_TILE];                  // the row's powers first (independent reads), then the fold from registers
#pragma unroll
                for (int i = 0; i < lsp::KX_TILE; ++i) pv[i] = row[i];
#pragma unroll
                for (int i = 0; i < lsp::KX_TILE; ++i) {
                    if (i < cnt) {
                        const int kx = kx0 + i;
                        if (q2 + kx * kx > s * (s + 1)) { row[nrun++] = run; run = 0.0f; ++s; }
                        run = run + pv[i];
                    }
                }
                row[nrun++] = run;
                nr[tid] = nrun;
            }
            __syncthreads();
            if (tid < S) {
                // every read is unconditional (a clamped index), so the reads of several rows go out together; the adds keep their order
#pragma unroll 8
                for (int ky = 0; ky < H; ++ky) {
                    const int i = tid - s0[ky];
                    const bool hit = i >= 0 && i < nr[ky];
                    const float v = Pw[ky * lsp::PITCH + (hit ? i : 0)];
                    E = hit ? E + v : E;
                }
            }
            // (the next tile's row pass writes Rre / Rim only; its barrier orders this read before the next power store)
        }
        if (tid < S) out[fi * S + tid] = E;
    }
}

// The same plane with a DCT-II along y (DY), along x (DX) or both (the statement: include/lns.h, "a basis per axis").
// A DCT axis of length N contracts against t_N[r] = cospi(r / 2N) read at (m (2 n + 1)) mod 4 N and has no imaginary part:
//   DX        W columns instead of W / 2 + 1, Rre only
//   DY        re = chain t_H . Rre, im = chain t_H . Rim (if Rim exists)
//   DFT y, DX the two segments of spectrum_plane without their Rim terms: re = chain cos . Rre, im = chain (-sin) . Rre
// Shells count half cycles (lsp::half_y / half_x).  With DY and a DFT x the shell can rise by two per column: the runs of
// a row go to slot (shell - first shell) of a RUNS_WIDE row in Rre | Rim, skipped shells as zero runs (E + 0 = E, E >= +0);
// otherwise the shell rises by at most one per column and the runs are folded in place in Pw, as in spectrum_plane.
template <bool DY, bool DX>
__device__ __forceinline__ void spectrum_plane_basis(const float* f, const float* g, float* out, int H, int W, int S, float sd,
                                                     float mean, bool walls, bool clampv, float lo, float hi, float* sm) {
#pragma clang fp contract(off)
    constexpr bool RIM = !DX;                    // the row pass has an imaginary part
    constexpr bool FIM = !(DY && DX);            // the transform has one
    constexpr bool WIDE = DY && !DX;
    constexpr int BY = DY ? lsp::DCT : lsp::DFT, BX = DX ? lsp::DCT : lsp::DFT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, kh = lane >> 5;
    const int HW = H * W, NX = lsp::columns(W, BX), xp = W | 1;
    const int MW = DX ? 4 * W : W, MH = DY ? 4 * H : H;          // table lengths
    const lsp::Lds L = lsp::lds_layout(H, W, BY, BX);
    float *X = sm + L.field, *Rre = sm + L.re, *Rim = sm + L.im, *Pw = sm + L.pw;
    float *cw = sm + L.cw, *sw = sm + L.sw, *ch = sm + L.ch, *sh = sm + L.sh;
    int *s0 = reinterpret_cast<int*>(sm + L.s0), *nr = reinterpret_cast<int*>(sm + L.n);
    float* runs = WIDE ? Rre : Pw;
    constexpr int RP = WIDE ? lsp::RUNS_WIDE : lsp::PITCH;
    if (DX) { for (int r = tid; r < MW; r += 256) cw[r] = cospif((float)r / (float)(2 * W)); }
    else { for (int r = tid; r < W; r += 256) { float s, c; sincospif(2.0f * (float)r / (float)W, &s, &c); cw[r] = c; sw[r] = -s; } }
    if (DY) { for (int r = tid; r < MH; r += 256) ch[r] = cospif((float)r / (float)(2 * H)); }
    else { for (int r = tid; r < H; r += 256) { float s, c; sincospif(2.0f * (float)r / (float)H, &s, &c); ch[r] = c; sh[r] = -s; } }
    const float inv = 1.0f / (float)HW;
    const int nf = g ? 3 : 1;
    for (int fi = 0; fi < nf; ++fi) {
        for (int i0 = tid; i0 < HW; i0 += 256 * 8) {
            float fv[8], gv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = min(i0 + u * 256, HW - 1);
                fv[u] = fi != 1 ? f[i] : 0.0f;
                gv[u] = fi != 0 ? g[i] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = i0 + u * 256;
                if (i < HW) {
                    const int r = i / W, cx = i - r * W;
                    const bool zero = walls && (r == 0 || r == H - 1 || cx == 0 || cx == W - 1);
                    float v;
                    if (fi == 0) v = score_denorm(fv[u], sd, mean, zero, clampv, lo, hi);
                    else {
                        const float q = score_denorm(gv[u], sd, mean, zero, clampv, lo, hi);
                        v = fi == 1 ? q : score_denorm(fv[u], sd, mean, zero, clampv, lo, hi) - q;
                    }
                    X[r * xp + cx] = v;
                }
            }
        }
        __syncthreads();
        float E = 0.0f;
        for (int kx0 = 0; kx0 < NX; kx0 += lsp::KX_TILE) {
            if (WIDE && kx0) __syncthreads();    // the row pass overwrites the previous tile's run sums
            // row pass: R[y][kx0 + 0 .. 31], x ascending in one chain per part
            for (int mt = wave; mt * 32 < H; mt += 4) {
                f32x16 are, aim;
#pragma unroll
                for (int r = 0; r < 16; ++r) { are[r] = 0.0f; aim[r] = 0.0f; }
                const int y = mt * 32 + l31;
                const bool yok = y < H;
                const float* xr = X + (yok ? y : 0) * xp;
                const int kx = kx0 + l31;
                int idx = DX ? (kx * (2 * kh + 1)) % MW : (kx * kh) % MW;
                const int step = DX ? (4 * kx) % MW : (2 * kx) % MW;
                for (int x0 = 0; x0 < W; x0 += 2) {
                    const int x = x0 + kh;
                    const bool xok = x < W;
                    float av = xr[xok ? x : 0], bc = cw[idx];
                    av = (yok && xok) ? av : 0.0f; bc = xok ? bc : 0.0f;
                    are = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bc, are, 0, 0, 0);
                    if (RIM) {
                        float bs = sw[idx];
                        bs = xok ? bs : 0.0f;
                        aim = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bs, aim, 0, 0, 0);
                    }
                    idx += step; if (idx >= MW) idx -= MW;
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int yy = mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                    if (yy < H) { Rre[yy * lsp::PITCH + l31] = are[r]; if (RIM) Rim[yy * lsp::PITCH + l31] = aim[r]; }
                }
            }
            __syncthreads();
            for (int mt = wave; mt * 32 < H; mt += 4) {
                f32x16 fre, fim;
#pragma unroll
                for (int r = 0; r < 16; ++r) { fre[r] = 0.0f; fim[r] = 0.0f; }
                const int ky = mt * 32 + l31;
                const int step = DY ? (4 * ky) % MH : (2 * ky) % MH;
                int idx = DY ? (ky * (2 * kh + 1)) % MH : (ky * kh) % MH;
                for (int y0 = 0; y0 < H; y0 += 2) {
                    const int y = y0 + kh;
                    const bool ok = y < H;
                    const int ro = (ok ? y : 0) * lsp::PITCH + l31;
                    float ac = ch[idx], br = Rre[ro];
                    ac = ok ? ac : 0.0f; br = ok ? br : 0.0f;
                    fre = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, br, fre, 0, 0, 0);
                    if (RIM) {
                        float bi = Rim[ro];
                        bi = ok ? bi : 0.0f;
                        fim = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, bi, fim, 0, 0, 0);
                    }
                    idx += step; if (idx >= MH) idx -= MH;
                }
                if (!DY) {
                    idx = (ky * kh) % MH;
                    for (int y0 = 0; y0 < H; y0 += 2) {
                        const int y = y0 + kh;
                        const bool ok = y < H;
                        const int ro = (ok ? y : 0) * lsp::PITCH + l31;
                        float am = sh[idx], br = Rre[ro];
                        am = ok ? am : 0.0f; br = ok ? br : 0.0f;
                        if (RIM) {
                            float bi = Rim[ro];
                            bi = ok ? bi : 0.0f;
                            fre = __builtin_amdgcn_mfma_f32_32x32x2f32(-am, bi, fre, 0, 0, 0);
                        }
                        fim = __builtin_amdgcn_mfma_f32_32x32x2f32(am, br, fim, 0, 0, 0);
                        idx += step; if (idx >= MH) idx -= MH;
                    }
                }
                const int kxx = kx0 + l31;
                const int wx = lsp::weight_x(kxx, W, BX);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int kyy = mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                    const float wgt = (float)(lsp::weight_y(kyy, BY) * wx);
                    float p = 0.0f;
                    if (kxx < NX) {
                        const float a = fre[r] * inv;
                        const float aa = a * a;
                        if (FIM) {
                            const float b = fim[r] * inv;
                            const float bb = b * b;
                            p = wgt * (aa + bb);
                        } else p = wgt * aa;
                    }
                    if (kyy < H) Pw[kyy * lsp::PITCH + l31] = p;
                }
            }
            __syncthreads();
            // runs of equal shell along row ky, ascending kx: run (shell - first shell) of the row, skipped shells zero
            if (tid < H) {
                const int q = lsp::half_y(tid, H, BY), q2 = q * q;
                const int cnt = min(lsp::KX_TILE, NX - kx0);
                const float* row = Pw + tid * lsp::PITCH;
                float* rr = runs + tid * RP;
                const int qx0 = lsp::half_x(kx0, BX);
                const int sb = lsp::shell(q2 + qx0 * qx0);
                int s = sb;
                float run = 0.0f;
                s0[tid] = sb;
                float pv[lsp::KX_TILE];
#pragma unroll
                for (int i = 0; i < lsp::KX_TILE; ++i) pv[i] = row[i];
#pragma unroll
                for (int i = 0; i < lsp::KX_TILE; ++i) {
                    if (i < cnt) {
                        const int qx = lsp::half_x(kx0 + i, BX);
                        const int r2 = q2 + qx * qx;
                        // along a row sqrt(r2) rises by at most the column's step in half units (2 for a DFT x, else 1), and so
                        // does its rounding: at most two closures (WIDE) or one, i.e. s - sb <= 62 < RUNS_WIDE or <= 31 < PITCH
                        if (r2 > s * (s + 1)) { rr[s - sb] = run; run = 0.0f; ++s; }
                        if (WIDE && r2 > s * (s + 1)) { rr[s - sb] = 0.0f; ++s; }
                        run = run + pv[i];
                    }
                }
                rr[s - sb] = run;
                nr[tid] = s - sb + 1;
            }
            __syncthreads();
            if (tid < S) {
#pragma unroll 8
                for (int ky = 0; ky < H; ++ky) {
                    const int i = tid - s0[ky];
                    const bool hit = i >= 0 && i < nr[ky];
                    const float v = runs[ky * RP + (hit ? i : 0)];
                    E = hit ? E + v : E;
                }
            }
            // (not WIDE: the next tile's row pass writes Rre / Rim only; its barrier orders this read before the next power store)
        }
        if (tid < S) out[fi * S + tid] = E;
    }
}

// one of the four bases, chosen per launch (uniform): DFT / DFT is spectrum_plane itself
__device__ __forceinline__ void spectrum_plane_any(int basis, const float* f, const float* g, float* out, int H, int W, int S,
                                                   const ChannelNorm& D, float* sm) {
    switch (basis) {
    case 0: spectrum_plane(f, g, out, H, W, S, D.sd, D.mean, D.walls, D.clampv, D.lo, D.hi, sm); break;
    case 1: spectrum_plane_basis<true, false>(f, g, out, H, W, S, D.sd, D.mean, D.walls, D.clampv, D.lo, D.hi, sm); break;
    case 2: spectrum_plane_basis<false, true>(f, g, out, H, W, S, D.sd, D.mean, D.walls, D.clampv, D.lo, D.hi, sm); break;
    default: spectrum_plane_basis<true, true>(f, g, out, H, W, S, D.sd, D.mean, D.walls, D.clampv, D.lo, D.hi, sm); break;
    }
}

// frames [kk][B][C][H*W] (a decode stream's frame buffer): block q = (i * B + b) * C + c takes step j = sel[i] of the group
__global__ __launch_bounds__(256) void spectrum_group_kernel(SpectrumArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int q = blockIdx.x;
    const int c = q % a.C, s = q / a.C, b = s % a.B, i = s / a.B;
    const int j = a.sel[i];
    const long HW = (long)a.H * a.W;
    const float* f = a.frames + (((long)j * a.B + b) * a.C + c) * HW;
    const float* g = a.y ? a.y + (((long)b * a.y_T + a.y_t + j) * a.C + c) * HW : nullptr;
    float* out = a.out + (((long)b * a.o_T + a.o_t + i) * a.C + c) * a.K * a.S;
    const ChannelNorm D(a.norm, c);
    spectrum_plane_any(a.basis, f, g, out, a.H, a.W, a.S, D, reinterpret_cast<float*>(smem));
}

// stored fields yhat / y [B][T][C][H*W]: block = plane
__global__ __launch_bounds__(256) void spectrum_stored_kernel(SpectrumArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const long p = blockIdx.x;
    const int c = (int)(p % a.C);
    const long HW = (long)a.H * a.W;
    const ChannelNorm D(a.norm, c);
    spectrum_plane_any(a.basis, a.frames + p * HW, a.y ? a.y + p * HW : nullptr, a.out + p * a.K * a.S, a.H, a.W, a.S, D,
                       reinterpret_cast<float*>(smem));
}

static bool spectrum_args_ok(const SpectrumArgs& a) {
    if (a.basis < 0 || a.basis > 3) return false;
    return lsp::supported(a.H, a.W) && a.S == lsp::bins(a.H, a.W, a.basis & 1, a.basis >> 1) && a.S <= 256 && a.K == (a.y ? 3 : 1);
}

hipError_t launch_spectrum_group(const SpectrumArgs& a, hipStream_t s) {
    if (!spectrum_args_ok(a) || a.n < 1 || a.n > 8) return hipErrorInvalidValue;
    hipLaunchKernelGGL(spectrum_group_kernel, dim3((unsigned)((long)a.n * a.B * a.C)), dim3(256),
                       (size_t)lsp::lds_bytes(a.H, a.W, a.basis & 1, a.basis >> 1), s, a);
    return hipGetLastError();
}

hipError_t launch_spectrum_stored(const SpectrumArgs& a, hipStream_t s) {
    if (!spectrum_args_ok(a) || (long)a.n * a.B * a.C > 0x7fffffffL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(spectrum_stored_kernel, dim3((unsigned)((long)a.n * a.B * a.C)), dim3(256),
                       (size_t)lsp::lds_bytes(a.H, a.W, a.basis & 1, a.basis >> 1), s, a);
    return hipGetLastError();
}

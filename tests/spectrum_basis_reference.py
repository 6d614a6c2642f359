"""References of the energy spectra with a basis per axis (include/lns.h "energy spectra", "a basis per axis";
lns_op_energy_spectrum_basis, the option "spectrum_basis"), in numpy, with no GPU, no library and no FFT.

A basis is a pair (by, bx) of DFT = 0 / DCT = 1, y first; BASES lists the four, NEW the three that are not DFT / DFT.
`shell_map`, `bins`: the integer side -- shells in half cycles per side unless both axes are DFT.
`spectra64`: the ground truth -- the float64 transform of the statement's fp32 fields (spectrum_reference._fields: D_c in
fp32, the error differenced per pixel in fp32) as dense cosine / sine matrices whose arguments are reduced in integers first.
For DFT / DFT it reproduces spectrum_reference.spectra64 (numpy.fft) to 1e-11.
`spectra32`: the project's "own" -- the kernel's algorithm in float32 numpy with sequential k: row pass over x, column pass
over y (one chain per part, the DFT y axis in its two segments), power, shell sums in row-major order.  It is not held to
the kernel bit for bit; it measures what fp32 can do on an input, which is what makes a tolerance admissible (3 x own).
`cases(H, W)`: spectrum_reference.cases plus a cosine-synthesised steep truth (amplitude (1 + k)^-3 per DCT mode, k in
cycles per side: a field with walls and no jump in the mirror extension), under both normalisations.

Layouts and `norm`: as spectrum_reference."""
import numpy as np

import spectrum_reference as sr

DFT, DCT = 0, 1
BASES = ((DFT, DFT), (DCT, DFT), (DFT, DCT), (DCT, DCT))
NEW = BASES[1:]
NAMES = {(DFT, DFT): "dft,dft", (DCT, DFT): "dct,dft", (DFT, DCT): "dft,dct", (DCT, DCT): "dct,dct"}
REL, ABS = sr.REL, sr.ABS


def columns(W, bx):
    return W if bx == DCT else W // 2 + 1


def half_counts(H, W, by, bx):
    """([H], [NX]) half-cycle counts of the stored rows and columns: a DCT index m counts m, a DFT wavenumber k counts 2 k."""
    ky = np.arange(H)
    qy = ky if by == DCT else 2 * np.where(ky <= H // 2, ky, ky - H)
    kx = np.arange(columns(W, bx))
    qx = kx if bx == DCT else 2 * kx
    return qy, qx


def shell_map(H, W, by, bx):
    """[H, NX] int shell of every stored mode and the weights wy [H], wx [NX]."""
    if (by, bx) == (DFT, DFT):
        s, w = sr.shell_map(H, W)
        return s, np.ones(H), w
    qy, qx = half_counts(H, W, by, bx)
    r2 = qy[:, None] ** 2 + qx[None, :] ** 2
    s = np.array([[sr.shell(v) for v in row] for row in r2], dtype=np.int64)
    wy = np.ones(H)
    if by == DCT:
        wy = np.where(np.arange(H) == 0, 1.0, 2.0)
    if bx == DCT:
        wx = np.where(np.arange(W) == 0, 1.0, 2.0)
    else:
        wx = sr.shell_map(H, W)[1]
    return s, wy, wx


def bins(H, W, by, bx):
    if (by, bx) == (DFT, DFT):
        return sr.bins(H, W)
    qy = H - 1 if by == DCT else 2 * (H // 2)
    qx = W - 1 if bx == DCT else 2 * (W // 2)
    return sr.shell(qy * qy + qx * qx) + 1


def bins_brute(H, W, by, bx):
    """S as the largest shell any stored mode falls into, plus one."""
    return int(shell_map(H, W, by, bx)[0].max()) + 1


def tables(N, basis, ncoef, dtype):
    """(cos [ncoef, N], -sin [ncoef, N] or None): the matrix of an axis of length N, argument reduced in integers first."""
    k, n = np.arange(ncoef)[:, None], np.arange(N)[None, :]
    if basis == DCT:
        return np.cos(np.pi * ((k * (2 * n + 1)) % (4 * N)) / (2.0 * N)).astype(dtype), None
    a = 2.0 * np.pi * ((k * n) % N) / N
    return np.cos(a).astype(dtype), (-np.sin(a)).astype(dtype)


def _shell_sum(p, s, S, dtype):
    lead = p.shape[:-2]
    flat = p.reshape((-1, s.size))
    out = np.zeros((flat.shape[0], S), dtype=dtype)
    idx = s.reshape(-1)
    for i in range(flat.shape[0]):
        np.add.at(out[i], idx, flat[i])
    return out.reshape(lead + (S,))


def transform64(u, by, bx):
    """(re, im or None) [..., H, NX] float64 of u [..., H, W]."""
    H, W = u.shape[-2:]
    u = u.astype(np.float64)
    cx, mx = tables(W, bx, columns(W, bx), np.float64)
    cy, my = tables(H, by, H, np.float64)
    rre = u @ cx.T
    rim = u @ mx.T if mx is not None else None
    if by == DCT:
        return cy @ rre, (cy @ rim if rim is not None else None)
    if rim is None:
        return cy @ rre, my @ rre
    return cy @ rre - my @ rim, cy @ rim + my @ rre


def spectra64(y_hat, y=None, basis=(DFT, DFT), denorm_dtype=np.float32, **norm):
    """[B, T, C, K, S] float64, K = 3 (forecast, truth, error) or 1 (y None)."""
    by, bx = basis
    H, W = y_hat.shape[-2:]
    s, wy, wx = shell_map(H, W, by, bx)
    S = bins(H, W, by, bx)
    rows = []
    for u in sr._fields(y_hat, y, norm, denorm_dtype):
        re, im = transform64(u, by, bx)
        p = (re / float(H * W)) ** 2
        if im is not None:
            p = p + (im / float(H * W)) ** 2
        rows.append(_shell_sum(p * (wy[:, None] * wx[None, :]), s, S, np.float64))
    return np.stack(rows, axis=-2)


def spectra32(y_hat, y=None, basis=(DFT, DFT), **norm):
    """The kernel's algorithm in float32 with sequential k."""
    f32 = np.float32
    by, bx = basis
    H, W = y_hat.shape[-2:]
    NX = columns(W, bx)
    s, wy, wx = shell_map(H, W, by, bx)
    S = bins(H, W, by, bx)
    cx, mx = tables(W, bx, NX, f32)           # [NX, W]
    cy, my = tables(H, by, H, f32)            # [H, H]
    inv = f32(1.0) / f32(H * W)
    wgt = (wy[:, None] * wx[None, :]).astype(f32)
    rows = []
    for u in sr._fields(y_hat, y, norm, f32):
        lead = u.shape[:-2]
        rre = np.zeros(lead + (H, NX), f32)
        rim = np.zeros(lead + (H, NX), f32) if mx is not None else None
        for x in range(W):
            ux = u[..., :, x, None]
            rre += ux * cx[:, x]
            if rim is not None:
                rim += ux * mx[:, x]
        re = np.zeros(lead + (H, NX), f32)
        im = np.zeros(lead + (H, NX), f32) if (rim is not None or by == DFT) else None
        for yy in range(H):
            c = cy[:, yy][:, None]
            re += c * rre[..., yy, None, :]
            if rim is not None:
                im += c * rim[..., yy, None, :]
        if by == DFT:
            for yy in range(H):
                m = my[:, yy][:, None]
                if rim is not None:
                    re += (-m) * rim[..., yy, None, :]
                im += m * rre[..., yy, None, :]
        a = re * inv
        p = a * a
        if im is not None:
            b = im * inv
            p = p + b * b
        rows.append(_shell_sum((wgt * p).astype(f32), s, S, f32))
    return np.stack(rows, axis=-2)


def bound(e64):
    return sr.bound(e64)


def worst_ratio(e, e64):
    return sr.worst_ratio(e, e64)


def steep_cos(rng, shape, H, W):
    """Cosine-synthesised fields: DCT-II modes (my, mx) of random sign and size with amplitude (1 + k)^-3, k = the mode's
    wavenumber in cycles per side; unit standard deviation."""
    ty, _ = tables(H, DCT, H, np.float64)
    tx, _ = tables(W, DCT, W, np.float64)
    k = 0.5 * np.sqrt(np.arange(H)[:, None] ** 2.0 + np.arange(W)[None, :] ** 2.0)
    A = (1.0 + k) ** -3.0 * rng.standard_normal(shape + (H, W))
    u = ty.T @ A @ tx
    sd = u.std(axis=(-2, -1), keepdims=True)
    return u / np.where(sd > 0, sd, 1.0)


def cases(H, W):
    """spectrum_reference.cases(H, W) followed by the cosine-synthesised steep truth under both normalisations."""
    out = list(sr.cases(H, W))
    amp = np.asarray(sr.PERTURBATIONS, np.float64).reshape(sr.B, sr.T, 1, 1, 1)
    for ni, norm in enumerate(sr.NORMS):
        rng = np.random.default_rng(1000 * H + 10 * W + 4 + ni)
        y = steep_cos(rng, (sr.B, sr.T, sr.C), H, W)
        y_hat = y + amp * rng.standard_normal((sr.B, sr.T, sr.C, H, W))
        out.append(("steep-cos %dx%d mean=%g std=%g" % (H, W, norm["mean"], norm["std"]),
                    y_hat.astype(np.float32), y.astype(np.float32), norm))
    return out


def wall_mode(H, W, my, kx):
    """cos(pi my (y + 1/2) / H) cos(2 pi kx x / W), float64 [H, W]: one DCT-II mode in y times one Fourier mode in x."""
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return np.cos(np.pi * my * (yy + 0.5) / H) * np.cos(2.0 * np.pi * kx * xx / W)


def ramp(H, W):
    """(y / H) (1 + 0.5 cos(2 pi 3 x / W)): a ramp in the non-periodic axis."""
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return (yy / float(H)) * (1.0 + 0.5 * np.cos(2.0 * np.pi * 3.0 * xx / W))

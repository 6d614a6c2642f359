"""The localised ensemble transform Kalman filter of include/lns.h ("localised ensemble transform Kalman filter") stated on its own
in numpy, for the tests.  Two statements:

* the INDEPENDENT one (`local_analysis`): for every domain l the filter of tests/etkf_reference.py under the per-value weights
  rinv_p * rho(l, patch(p)) -- the anomalies of etkf_reference's step 1, its `transform` and `update` (and, in the tests, its
  `kalman`) -- and the result taken at latent pixel l.  There are no patch sums in it.  (etkf_reference.gram rounds its weights
  to float32, which a product with the taper is not; so the weighted sums over the values are written here, in the dtype asked
  for, from the same anomalies.)  float64 and np.longdouble.
* the ORDER-EXACT one in float64 of what the device does behind the patch Gram: `taper` / `weights` (step 3), `combine` (step 4: acc
  = acc + rho * G over steps and patches, ascending, unfused) and `update_local` (step 6), which the bit tests use; `patch_gram`
  (step 2) is etkf_reference.gram on the values of one patch at a time.

The tolerance rule is etkf_reference's: max(1e-12, 3 x own), own = the float64 form against the longdouble form.

Layouts: frames [n, B, M, C, H, W], y [B, n, C, H, W], rinv broadcastable to [B, n, C, H, W]; part [B, n, h*w, M*M + M + 3];
S_local [B, h*w, M, M], g_local [B, h*w, M]; X_local [B, h*w, M, M]; z [B, M, c, h, w]; bc = (bc_y, bc_x), 0 periodic, 1 wall."""
import numpy as np

import etkf_reference as er
from ensemble_exceed_reference import denorm

LD = er.LD
PERIODIC, WALL = 0, 1


# ---- 1. patches ----------------------------------------------------------------------------------------------------------------
def patch_index(H, W, h, w, mistake=None):
    """[H, W] int: the patch ty * w + tx of pixel (y, x), ty = (y * h) // H, tx = (x * w) // W.  mistake "tytx_swapped": the row index
    from x and the column index from y."""
    y, x = np.arange(H)[:, None], np.arange(W)[None, :]
    if mistake == "tytx_swapped":
        return ((x * h) // W) * w + (y * w) // H
    return ((y * h) // H) * w + (x * w) // W + 0 * x


# ---- 3. the taper --------------------------------------------------------------------------------------------------------------
def taper(r, dt=np.float64):
    """Gaspari-Cohn at r >= 0 in dtype dt, in the order of the statement"""
    r = np.asarray(r, dtype=dt)
    c53, c58, c112 = dt(5) / dt(3), dt(5) / dt(8), dt(1) / dt(12)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        r2 = r * r
        r3 = r2 * r
        r4 = r3 * r
        r5 = r4 * r
        near = (((dt(1) - c53 * r2) + c58 * r3) + dt(0.5) * r4) - dt(0.25) * r5
        far = (((((dt(4) - dt(5) * r) + c53 * r2) + c58 * r3) - dt(0.5) * r4) + c112 * r5) - dt(2) / (dt(3) * r)
    far = np.where(far > 0, far, dt(0))
    return np.where(r >= 2, dt(0), np.where(r <= 1, near, far)).astype(dt)


def weights(h, w, radius, bc, dt=np.float64, mistake=None):
    """rho [h*w (domain l), h*w (patch t)] in dt.  mistake: "wrap_on_wall" (every axis wraps), "taper_twice" (rho squared)."""
    i, j = np.divmod(np.arange(h * w), w)
    dy, dx = np.abs(i[:, None] - i[None, :]), np.abs(j[:, None] - j[None, :])
    if bc[0] == PERIODIC or mistake == "wrap_on_wall":
        dy = np.minimum(dy, h - dy)
    if bc[1] == PERIODIC or mistake == "wrap_on_wall":
        dx = np.minimum(dx, w - dx)
    dist = np.sqrt((dy * dy + dx * dx).astype(dt))
    rho = taper(dist / dt(radius), dt)
    return rho * rho if mistake == "taper_twice" else rho


# ---- 2. the patch sums (through etkf_reference.gram) -----------------------------------------------------------------------------
def patch_gram(frames, y, rinv, grid, norm=None, dt=np.float64):
    """-> part [B, n, h*w, M*M + M + 3] in dt: etkf_reference.gram on the values of patch t alone, for every t.  (A patch is a
    rectangle of the plane; the frames are denormalised once, as whole frames -- the wall rows are the frame's -- and the Gram
    takes the rectangle of the denormalised float32 values as they are.)"""
    frames = np.asarray(frames, dtype=np.float32)
    n, B, M, C, H, W = frames.shape
    h, w = grid
    r = np.broadcast_to(np.asarray(rinv, dtype=np.float32), (B, n, C, H, W))
    v, q = denorm(frames, norm), denorm(y, norm)
    pidx = patch_index(H, W, h, w)
    part = np.zeros((B, n, h * w, M * M + M + 3), dtype=dt)
    for t in range(h * w):
        ys, xs = np.nonzero(pidx == t)
        if ys.size == 0:
            continue
        ry, rx = slice(ys.min(), ys.max() + 1), slice(xs.min(), xs.max() + 1)
        assert (pidx[ry, rx] == t).all() and (ry.stop - ry.start) * (rx.stop - rx.start) == ys.size
        S, g, stat = er.gram(v[..., ry, rx], q[..., ry, rx], r[..., ry, rx], None, dt)
        part[:, :, t, :M * M] = S.reshape(B, n, M * M)
        part[:, :, t, M * M:M * M + M] = g
        part[:, :, t, M * M + M:] = stat
    return part


# ---- 4. the local sums, in the device's order -------------------------------------------------------------------------------------
def combine(part, grid, radius, bc, M, dt=np.float64):
    """part [B, n, h*w, E] -> (S_local [B, h*w, M, M], g_local [B, h*w, M], S_glob [B, M, M], g_glob [B, M], stat [B, n, 3]): acc = acc +
    rho * G over the steps, then the patches with rho > 0, ascending, unfused; the global sums with rho = 1; stat per step.  The upper
    triangle is summed and mirrored."""
    part = np.asarray(part, dtype=dt)
    B, n, hw, E = part.shape
    h, w = grid
    assert hw == h * w and E == M * M + M + 3
    rho = weights(h, w, radius, bc, dt)
    loc = np.zeros((B, hw, M * M + M), dtype=dt)
    glob = np.zeros((B, M * M + M), dtype=dt)
    stat = np.zeros((B, n, 3), dtype=dt)
    for i in range(n):
        for t in range(hw):
            G = part[:, i, t, :M * M + M]
            glob = glob + dt(1) * G
            stat[:, i] = stat[:, i] + part[:, i, t, M * M + M:]
            for l in range(hw):
                if rho[l, t] > 0:
                    loc[:, l] = loc[:, l] + rho[l, t] * G
    iu = np.triu_indices(M)

    def sym(flat):
        S = flat.reshape(flat.shape[:-1] + (M, M)).copy()
        S[..., iu[1], iu[0]] = S[..., iu[0], iu[1]]
        return S
    return sym(loc[..., :M * M]), loc[..., M * M:].copy(), sym(glob[..., :M * M]), glob[..., M * M:].copy(), stat


def transform_local(S_local, g_local, rho_infl, dt=np.float64):
    """etkf_reference.transform per domain: -> (X [B, hw, M, M], wbar [B, hw, M], lam [B, hw, M], status [B, hw])"""
    B, hw, M, _ = S_local.shape
    X, wbar, lam, status, _ = er.transform(np.asarray(S_local).reshape(B * hw, 1, M, M), np.asarray(g_local).reshape(B * hw, 1, M), rho_infl, dt)
    return X.reshape(B, hw, M, M), wbar.reshape(B, hw, M), lam.reshape(B, hw, M), status.reshape(B, hw)


# ---- 6. the update ----------------------------------------------------------------------------------------------------------------
def update_local(z, X_local, dt=np.float64, rounded=True, mistake=None):
    """z [B, M, c, h, w] float32, X_local [B, h*w, M, M]: etkf_reference.update of latent pixel l under X_local[:, l].  mistake
    "neighbour_X": pixel l under the transform of pixel l + 1."""
    z = np.asarray(z, dtype=np.float32)
    B, M, c, h, w = z.shape
    zz = z.reshape(B, M, c, h * w)
    out = np.zeros(zz.shape, dtype=np.float32 if rounded else dt)
    for l in range(h * w):
        src = (l + 1) % (h * w) if mistake == "neighbour_X" else l
        out[:, :, :, l] = er.update(zz[:, :, :, l], np.asarray(X_local)[:, src], dt, rounded=rounded)
    return out.reshape(z.shape)


# ---- the independent statement -----------------------------------------------------------------------------------------------------
def weighted_sums(frames, y, rinv, wmap, norm=None, dt=np.float64):
    """S [B, M, M], g [B, M] over ALL steps and values under the weights rinv_p * wmap_p (wmap [C, H, W] in dt), from the anomalies of
    etkf_reference's step 1; a value with !(rinv > 0) or wmap = 0 is selected out."""
    frames, y = np.asarray(frames, dtype=np.float32), np.asarray(y, dtype=np.float32)
    n, B, M, C, H, W = frames.shape
    r = np.broadcast_to(np.asarray(rinv, dtype=np.float32), (B, n, C, H, W))
    v, q = denorm(frames, norm), denorm(y, norm)
    S, g = np.zeros((B, M, M), dtype=dt), np.zeros((B, M), dtype=dt)
    wm = np.asarray(wmap, dtype=dt).reshape(-1)
    for b in range(B):
        for i in range(n):
            with np.errstate(invalid="ignore"):
                sel = (r[b, i] > 0).reshape(-1) & (wm > 0)
            f = v[i, b].reshape(M, -1)[:, sel].astype(dt)
            yy = q[b, i].reshape(-1)[sel].astype(dt)
            ww = r[b, i].reshape(-1)[sel].astype(dt) * wm[sel]
            ybar = f[0].copy()
            for m in range(1, M):
                ybar = ybar + f[m]
            ybar = ybar / dt(M)
            Y, d = f - ybar, yy - ybar
            Yw = Y * ww
            Si = Yw @ Y.T
            S[b] = S[b] + (np.triu(Si) + np.triu(Si, 1).T)
            g[b] = g[b] + Yw @ d
    return S, g


def local_analysis(frames, y, rinv, z, rho_infl, grid, radius, bc, norm=None, dt=np.float64, mistake=None):
    """For every domain l: the weights rinv_p * rho(l, patch(p)), etkf_reference.transform on their sums, etkf_reference.update of
    latent pixel l.  -> dict(S, g, X, wbar, lam, status (per domain), z [B, M, c, h, w] unrounded in dt).  mistake: one of
    "tytx_swapped", "wrap_on_wall", "taper_twice", "neighbour_X"."""
    frames = np.asarray(frames, dtype=np.float32)
    n, B, M, C, H, W = frames.shape
    h, w = grid
    hw = h * w
    pidx = patch_index(H, W, h, w, mistake)
    rho = weights(h, w, radius, bc, dt, mistake)
    S, g = np.zeros((B, hw, M, M), dtype=dt), np.zeros((B, hw, M), dtype=dt)
    for l in range(hw):
        wmap = np.broadcast_to(rho[l][pidx][None], (C, H, W))
        S[:, l], g[:, l] = weighted_sums(frames, y, rinv, wmap, norm, dt)
    X, wbar, lam, status = transform_local(S, g, rho_infl, dt)
    return dict(S=S, g=g, X=X, wbar=wbar, lam=lam, status=status, z=update_local(z, X, dt, rounded=False, mistake=mistake))


def exact_analysis(frames, y, rinv, z, rho_infl, grid, radius, bc, norm=None):
    """The device's route in float64: patch sums, combine, transform per domain, update -> the dict of local_analysis plus the global
    Xg, wbarg, lamg, statusg, stat and part"""
    M = np.asarray(frames).shape[2]
    part = patch_gram(frames, y, rinv, grid, norm)
    S, g, Sg, gg, stat = combine(part, grid, radius, bc, M)
    X, wbar, lam, status = transform_local(S, g, rho_infl)
    Xg, wbarg, lamg, statusg, _ = er.transform(Sg[:, None], gg[:, None], rho_infl)
    return dict(S=S, g=g, X=X, wbar=wbar, lam=lam, status=status, z=update_local(z, X, rounded=False), Xg=Xg, wbarg=wbarg, lamg=lamg,
                statusg=statusg, stat=stat, part=part)

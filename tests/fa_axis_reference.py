"""float64 statements of the kernels that build a FABlock's Kx / Ky (fa_reducer*, fa_lrk*), of the SABlock pre-norm (ln_pe) and
of the GroupNorm materialisation (apply), and the input sets the CPU and the GPU tests share.

    reducer   u = W2 gelu(W1 LayerNorm(W_in m)) + b2 on pooled rows m [B, n, C]: LayerNorm over C with eps 1e-5 and the biased
              variance, the exact (erf) GELU; u [B, Out, n] as the kernels store it
    lrk       q, k = the halves of qk [B, 2 heads DK, n]; rotary as the reference defines it -- pos = torch.linspace(0, 1, n,
              float32) on the CPU, the angle is the float32 product (pos * 64) * inv_freq, cos and sin are taken in float64 --
              and K[b][h] = q' k'^T, no softmax and no scaling
    ln_pe     h[b][c][i] = LayerNorm_c(x[b][:][i]) gamma[c] + beta[c] + pe[i][c]
    apply     y = act(x scale + shift), act 0 none, 1 swish, 2 gelu (erf), 3 relu, 4 tanh, 5 sigmoid

Errors are relative L2 per sample; for K per (sample, head), because one bad head of eight disappears in a sample's figure.

Tolerances.  KERNEL_TOL = 2e-6 is the project's op-level tolerance (tests/test_gpu_parity.py) and holds wherever nothing else
is said; the float32 CPU oracle stays within ORACLE_TOL = 5e-7 of these statements on every zero-mean set
(tests/test_fa_axis_cpu.py).  Two families have no number fixed in advance, because the conditioning of the inputs sets what
float32 can reach: the reducer on rows with a per-channel offset (`offset`: up to +-3 per channel of the pooled rows;
`ln_offset`: the offset that to_in turns into a common value, so that LayerNorm subtracts a mean of up to three standard
deviations -- the first kind alone does not reach LayerNorm, see reducer_input) and the low-rank kernel (q scaled by 1e-4, k by 3e3, angles of up to 640 rad).  Their tolerance is TOL_FACTOR = 4
times the oracle's own float32-against-float64 error on the same set, worst sample (worst (sample, head)) of the set: the
device's k-pair MFMA order and the oracle's sequential order are two independent float32 orders of similar size.  The oracle
takes its rotary positions from numpy's linspace, an ulp away from torch's at some positions; its error is therefore measured
against the statement evaluated on the oracle's own positions (positions()), so that the figure is float32 rounding and not
a difference of definitions multiplied by the angle scale.
tools/fa_axis_parity.py writes the measured oracle errors and the tolerances to profiles/fa_axis_parity.json.

A constant pooled row: under a general to_in only the zero row is constant after to_in (W_in c 1 varies with the channel), so
the `const_row` sets zero one row per sample; LayerNorm maps it to beta exactly and the row of u must be the reducer's
W2 gelu(W1 beta) + b2."""
import functools

import numpy as np

from lns_amd import filler

KERNEL_TOL = 2e-6
ORACLE_TOL = 5e-7
TOL_FACTOR = 4.0
LN_EPS = 1e-5

# ---- shapes ----------------------------------------------------------------------------------------------------------------
# (B, n, C, Hid, Out)
REDUCER_MFMA = [(2, 32, 64, 128, 64),      # full blocks
                (5, 7, 64, 128, 64),       # block 0 spans five samples, block 1 has 3 live rows
                (3, 15, 32, 64, 32),       # ragged blocks
                (2, 33, 64, 128, 48),      # Out not a multiple of 32
                (2, 24, 32, 64, 200),      # second 128-chunk of the last GEMM, ragged
                (1, 96, 64, 128, 130)]     # second 128-chunk, ragged
REDUCER_SCALAR = [(3, 7, 24, 48, 16), (2, 20, 40, 80, 33)]        # C % 32 != 0: the scalar form
REDUCER_SHAPES = REDUCER_MFMA + REDUCER_SCALAR
# merged launches: (B, C, Hid, Out), (nx, ny)
REDUCER_MERGED = [((3, 64, 128, 64), (24, 48)), ((3, 32, 64, 32), (15, 30)), ((5, 64, 128, 48), (7, 15))]
KINDS = ("zero_mean", "offset", "ln_offset", "const_row")
MEASURED_KINDS = ("offset", "ln_offset")       # tolerance TOL_FACTOR x the oracle's own error
LN_SHIFTS = (3.0, -2.25, 1.5)                  # ln_offset: the LayerNorm mean of sample b, in standard deviations of its row
# (B, heads, DK, n)
LRK_SHAPES = [(2, 8, 128, 32),             # full tiles
              (2, 2, 64, 7),               # small n
              (3, 2, 64, 15),              # ragged
              (2, 8, 128, 33),             # one live row in the second tile
              (1, 8, 128, 96),             # larger n
              (1, 2, 128, 160),            # LDS exactly 160 KB
              (2, 2, 32, 48)]              # small DK
LRK_MERGED = [((2, 2, 64), (24, 48)), ((3, 2, 64), (7, 15))]       # (B, heads, DK), (nx, ny): LDS sized by the larger axis
FREQS = ("std", "x10")
Q_SCALE, K_SCALE = 1e-4, 3e3
# (B, C, n); C / 4 > 32 (160, 256) takes ln_pe's loop path
LNPE_SHAPES = [(2, 64, 256), (2, 128, 105), (3, 30, 70), (2, 5, 9), (2, 160, 64), (1, 256, 130)]
APPLY_HW = (1, 105, 256, 4097)
APPLY_MAGS = (1e-20, 1.0, 1e20)
CHAIN = dict(B=2, C=64, H=24, W=48, Out=64, heads=2, DK=64)


def rel_l2(got, ref, keep):
    """Relative L2 over every axis but the first `keep`: [B] for keep = 1, [B, heads] for keep = 2."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    ax = tuple(range(keep, ref.ndim))
    return np.sqrt(((got - ref) ** 2).sum(axis=ax) / (ref ** 2).sum(axis=ax))


def _erf(a):
    import torch
    return torch.special.erf(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))).numpy()


def gelu64(a):
    return 0.5 * a * (1.0 + _erf(a / np.sqrt(2.0)))


# ---- reducer ---------------------------------------------------------------------------------------------------------------
def reducer_weights(tag, C, Hid, Out, seed=1, kind=None):
    """A PoolingReducer's state_dict under the prefix `tag`, the deterministic filler at the oracle's scale.  kind ln_offset:
    to_in is I + that matrix -- its eigenvalues lie in a disc of radius 0.58 around 1, so the offset reducer_input solves for
    stays a few standard deviations per channel and the cancellation is LayerNorm's, not the to_in GEMM's (with the plain
    random matrix the solved offset is 28 .. 1350 times the rows)."""
    shapes = {".to_in.weight": (C, C), ".out_ffn.0.weight": (C,), ".out_ffn.0.bias": (C,), ".out_ffn.1.weight": (Hid, C),
              ".out_ffn.3.weight": (Out, Hid), ".out_ffn.3.bias": (Out,)}
    w = {tag + k: filler.fill_tensor("%s-%d-%d-%d%s" % (tag, C, Hid, Out, k), s, seed) for k, s in shapes.items()}
    if kind == "ln_offset":
        w[tag + ".to_in.weight"] = (w[tag + ".to_in.weight"] + np.eye(C, dtype=np.float32)).astype(np.float32)
    return w


def const_rows(B, n):
    """The zeroed row of each sample of a const_row set."""
    return [(3 * b + 1) % n for b in range(B)]


def reducer_input(kind, B, n, C, tag="x", seed=3, w_in=None):
    """w_in: the set's to_in matrix [C, C], needed by ln_offset."""
    m = filler.normal("m-%s-%s-%d-%d-%d" % (tag, kind, B, n, C), (B, n, C), seed)
    if kind == "offset":          # a per-(sample, channel) offset of up to +-3 standard deviations
        m = m + (filler.uniform01("off-%s-%d-%d-%d" % (tag, B, n, C), B * C, seed).reshape(B, 1, C) * 2 - 1) * np.float32(3.0)
    if kind == "ln_offset":
        # The offset above does not reach LayerNorm: a random to_in turns it into another zero-mean vector over the channels
        # (|mean| / std of a row after to_in is 0.06 .. 0.17 in the median, as on the zero-mean sets).  This kind adds the
        # per-channel offset that to_in maps to the SAME value on every channel, W_in off = a 1 with a = LN_SHIFTS[b % 3] standard
        # deviations of the rows after to_in: LayerNorm then subtracts a mean of up to three times what it keeps.
        t = m.astype(np.float64) @ w_in.astype(np.float64).T
        one = np.linalg.solve(w_in.astype(np.float64), np.ones(C))
        for b in range(B):
            m[b] = (m[b] + LN_SHIFTS[b % 3] * t[b].std() * one).astype(np.float32)
    if kind == "const_row":
        for b, i in enumerate(const_rows(B, n)):
            m[b, i] = 0.0
    return np.ascontiguousarray(m, dtype=np.float32)


def reducer64(m, w, tag):
    """[B, n, C] -> u [B, Out, n], float64."""
    f = lambda k: w[tag + k].astype(np.float64)
    t = m.astype(np.float64) @ f(".to_in.weight").T
    mean = t.mean(axis=-1, keepdims=True)
    var = ((t - mean) ** 2).mean(axis=-1, keepdims=True)
    t = (t - mean) / np.sqrt(var + LN_EPS) * f(".out_ffn.0.weight") + f(".out_ffn.0.bias")
    t = gelu64(t @ f(".out_ffn.1.weight").T)
    u = t @ f(".out_ffn.3.weight").T + f(".out_ffn.3.bias")
    return np.ascontiguousarray(u.transpose(0, 2, 1))


def reducer_oracle(m, w, tag):
    """lns_oracle._pooling_reducer after the pool: the rows enter as a [B, C, n, 1] field, whose mean over the last axis is
    the identity."""
    import lns_oracle
    x = np.ascontiguousarray(m.transpose(0, 2, 1)[..., None])
    return np.ascontiguousarray(lns_oracle._pooling_reducer(w, tag, x).transpose(0, 2, 1))


def reducer_beta_row64(w, tag):
    """What the reducer makes of a row LayerNorm maps to beta: [Out]."""
    f = lambda k: w[tag + k].astype(np.float64)
    return gelu64(f(".out_ffn.1.weight") @ f(".out_ffn.0.bias")) @ f(".out_ffn.3.weight").T + f(".out_ffn.3.bias")


def reducer_name(kind, B, n, C, Hid, Out, tag="x"):
    return "%s-%s-B%dn%dC%dH%dO%d" % (kind, tag, B, n, C, Hid, Out)


@functools.lru_cache(maxsize=None)
def reducer_set(kind, B, n, C, Hid, Out, tag="x"):
    """One axis of one launch: inputs, weights, the float64 statement, the oracle's error per sample and the tolerance."""
    w = reducer_weights(tag, C, Hid, Out, kind=kind)
    m = reducer_input(kind, B, n, C, tag, w_in=w[tag + ".to_in.weight"])
    ref = reducer64(m, w, tag)
    own = rel_l2(reducer_oracle(m, w, tag), ref, 1)
    tol = TOL_FACTOR * float(own.max()) if kind in MEASURED_KINDS else KERNEL_TOL
    for a in (m, ref, own, *w.values()):
        a.setflags(write=False)
    return dict(name=reducer_name(kind, B, n, C, Hid, Out, tag), kind=kind, B=B, n=n, C=C, Hid=Hid, Out=Out, tag=tag, m=m, w=w, ref=ref,
                oracle_err=own, tol=tol)


def reducer_sets():
    """Every axis set the GPU tests launch: (kind, B, n, C, Hid, Out, tag)."""
    out = [(k,) + s + ("x",) for s in REDUCER_SHAPES for k in KINDS]
    for (B, C, Hid, Out), (nx, ny) in REDUCER_MERGED:
        for k in KINDS:
            out += [(k, B, nx, C, Hid, Out, "x"), (k, B, ny, C, Hid, Out, "y")]
    return out


# ---- low-rank kernel -------------------------------------------------------------------------------------------------------
def inv_freq(kind, DK):
    """std: 10000^(-2i / DK), the RotaryEmbedding buffer; x10: ten times that, angles of up to 640 rad."""
    f = filler.inv_freq(DK)
    return f if kind == "std" else (f * np.float32(10.0)).astype(np.float32)


def positions(n, source="torch"):
    """The float32 positions of the rotary embedding.  torch: torch.linspace(0, 1, n, float32) on the CPU, what the reference
    defines and the statement uses.  oracle: numpy's linspace (zeros for n = 1), what lns_oracle._rotary uses -- an ulp away
    from torch's at some positions; the oracle's own float32 error is measured against the statement on ITS positions, or the
    figure would be a difference of definitions times the angle scale of 64 or 640, not a rounding error."""
    if source == "oracle":
        return np.linspace(0.0, 1.0, n, dtype=np.float32) if n > 1 else np.zeros(1, np.float32)
    import torch
    return torch.linspace(0, 1, n, dtype=torch.float32).numpy()


def rotary_angles(n, invf, source="torch"):
    """The float32 angles [n, DK / 2]: (positions * 64) * inv_freq, every product rounded to float32."""
    pos = positions(n, source)
    t = (pos * np.float32(64.0)).astype(np.float32)
    return (t[:, None] * invf[None, :].astype(np.float32)).astype(np.float32)


def lrk_input(B, heads, DK, n, tag="x", seed=5):
    qk = filler.normal("qk-%s-%d-%d-%d-%d" % (tag, B, heads, DK, n), (B, 2 * heads * DK, n), seed)
    qk[:, :heads * DK] *= np.float32(Q_SCALE)
    qk[:, heads * DK:] *= np.float32(K_SCALE)
    return np.ascontiguousarray(qk, dtype=np.float32)


def lrk64(qk, heads, DK, invf, source="torch"):
    """qk [B, 2 heads DK, n] -> K [B, heads, n, n], float64, on the positions of `source` (positions())."""
    B, _, n = qk.shape
    half = DK // 2
    f = rotary_angles(n, invf, source).astype(np.float64)               # [n, half]
    c, s = np.cos(f).T[None, None], np.sin(f).T[None, None]             # [1, 1, half, n]
    v = qk.astype(np.float64).reshape(B, 2, heads, DK, n)

    def rot(t):                                                         # [B, heads, DK, n]
        a, b = t[:, :, :half], t[:, :, half:]
        return np.concatenate([a * c - b * s, b * c + a * s], axis=2)
    q, k = rot(v[:, 0]), rot(v[:, 1])
    return np.einsum("bhdi,bhdj->bhij", q, k)


def lrk_oracle(qk, heads, DK, invf):
    """lns_oracle._low_rank_kernel on the same q and k: its to_qk is the identity (exact in float32) on u = qk^T."""
    import lns_oracle
    M = 2 * heads * DK
    sd = {"k.to_qk.weight": np.eye(M, dtype=np.float32), "k.pos_emb.inv_freq": invf}
    return lns_oracle._low_rank_kernel(sd, "k", np.ascontiguousarray(qk.transpose(0, 2, 1)), heads)


def lrk_name(freq, B, heads, DK, n, tag="x"):
    return "%s-%s-B%dh%dD%dn%d" % (freq, tag, B, heads, DK, n)


@functools.lru_cache(maxsize=None)
def lrk_set(freq, B, heads, DK, n, tag="x"):
    invf = inv_freq(freq, DK)
    qk = lrk_input(B, heads, DK, n, tag)
    ref = lrk64(qk, heads, DK, invf)
    own = rel_l2(lrk_oracle(qk, heads, DK, invf), lrk64(qk, heads, DK, invf, "oracle"), 2)       # on the oracle's positions
    for a in (qk, ref, own, invf):
        a.setflags(write=False)
    return dict(name=lrk_name(freq, B, heads, DK, n, tag), freq=freq, B=B, heads=heads, DK=DK, n=n, tag=tag, qk=qk, invf=invf, ref=ref,
                oracle_err=own, tol=TOL_FACTOR * float(own.max()))


def lrk_sets():
    out = [(f,) + s + ("x",) for s in LRK_SHAPES for f in FREQS]
    for (B, heads, DK), (nx, ny) in LRK_MERGED:
        for f in FREQS:
            out += [(f, B, heads, DK, nx, "x"), (f, B, heads, DK, ny, "y")]
    return out


# ---- ln_pe -----------------------------------------------------------------------------------------------------------------
def hot_tokens(B, n):
    return [(5 * b + 3) % n for b in range(B)]


@functools.lru_cache(maxsize=None)
def lnpe_set(B, C, n):
    """x [B, C, n]: rows with a per-(sample, channel) offset of up to +-3, and one one-hot token per sample -- LayerNorm maps it
    to sqrt(C - 1) on the hot channel, the extremal input of the planner's bound; sample 0's is on the channel of the largest
    |gamma|.  pe has 11 rows more than tokens."""
    tag = "lnpe-%d-%d-%d" % (B, C, n)
    x = filler.normal(tag, (B, C, n), 7) + (filler.uniform01(tag + "off", B * C, 7).reshape(B, C, 1) * 2 - 1) * np.float32(3.0)
    g = filler.fill_tensor(tag + ".ln.weight", (C,), 7)
    be = filler.fill_tensor(tag + ".ln.bias", (C,), 7)
    pe = filler.fill_tensor(tag + ".pe", (1, n + 11, C), 7)[0]
    for b, i in enumerate(hot_tokens(B, n)):
        x[b, :, i] = 0.0
        x[b, int(np.argmax(np.abs(g))) if b == 0 else (7 * b + 1) % C, i] = 4.0
    x = np.ascontiguousarray(x, dtype=np.float32)
    ref = {p: lnpe64(x, g, be, pe if p else None) for p in (False, True)}
    for a in (x, g, be, pe, *ref.values()):
        a.setflags(write=False)
    return dict(B=B, C=C, n=n, x=x, gamma=g, beta=be, pe=pe, ref=ref)


def lnpe64(x, g, be, pe, eps=LN_EPS):
    """x [B, C, n] -> h [B, C, n], float64; pe [pe_len, C] or None."""
    x = x.astype(np.float64)
    mean = x.mean(axis=1, keepdims=True)
    var = ((x - mean) ** 2).mean(axis=1, keepdims=True)
    h = (x - mean) / np.sqrt(var + eps) * g.astype(np.float64)[None, :, None] + be.astype(np.float64)[None, :, None]
    if pe is not None:
        h = h + pe[:x.shape[2]].astype(np.float64).T[None]
    return h


def lnpe_oracle(x, g, be, pe, eps=LN_EPS):
    import lns_oracle
    h = lns_oracle.layernorm(np.ascontiguousarray(x.transpose(0, 2, 1)), g, be, eps)         # [B, n, C]
    if pe is not None:
        h = h + pe[None, :x.shape[2]]
    return np.ascontiguousarray(h.transpose(0, 2, 1))


def lnpe_bound(C, g, be, pe):
    """The bound Planner::lower_sa hands the consumer, in float64 (the entry point reports the float32 evaluation)."""
    return np.sqrt(float(C)) * np.abs(g).max() + np.abs(be).max() + (np.abs(pe).max() if pe is not None else 0.0)


# ---- apply -----------------------------------------------------------------------------------------------------------------
def act64(v, act):
    with np.errstate(over="ignore"):
        if act == 1:
            return v / (1.0 + np.exp(-v))
        if act == 2:
            return gelu64(v)
        if act == 3:
            return np.maximum(v, 0.0)
        if act == 4:
            return np.tanh(v)
        if act == 5:
            return 1.0 / (1.0 + np.exp(-v))
    return v


def apply_input(B, C, HW, mag, seed=9):
    """x of magnitude `mag`, and a (scale, shift) table whose shift has x's magnitude (it would drown a small x otherwise)."""
    tag = "apply-%d-%d-%d" % (B, C, HW)
    x = (filler.normal(tag, (B, C, HW), seed).astype(np.float64) * mag).astype(np.float32)
    u = filler.uniform01(tag + "ss", 3 * B * C, seed).reshape(3, B, C)
    scale = (0.3 + 1.7 * u[0]) * np.where(u[2] < 0.5, -1.0, 1.0)
    shift = (2 * u[1] - 1) * mag
    return x, np.ascontiguousarray(np.stack([scale, shift], axis=-1), dtype=np.float32)


def apply64(x, ss, act):
    v = x.astype(np.float64)
    if ss is not None:
        v = v * ss[..., 0].astype(np.float64)[..., None] + ss[..., 1].astype(np.float64)[..., None]
    return act64(v, act)


# ---- the chain pool -> reducer -> to_qk -> low-rank kernel ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chain_set():
    """A FABlock's way from its normalised input to Kx / Ky at (2, 64, 24, 48): random weights at the oracle's scale, the
    float64 chain and its intermediates."""
    c = CHAIN
    B, C, H, W, Out, heads, DK = (c[k] for k in ("B", "C", "H", "W", "Out", "heads", "DK"))
    x = filler.normal("chain-x", (B, C, H, W), 11)
    u = filler.uniform01("chain-ss", 2 * B * C, 11).reshape(2, B, C)
    ss = np.ascontiguousarray(np.stack([0.5 + u[0], (2 * u[1] - 1) * 0.5], axis=-1), dtype=np.float32)
    w = {}
    for tag in ("x", "y"):
        w.update(reducer_weights("chain" + tag, C, 2 * C, Out, seed=2))
        w["chain%s.to_qk.weight" % tag] = filler.fill_tensor("chain%s.to_qk.weight" % tag, (2 * heads * DK, Out), 2)
    invf = inv_freq("std", DK)
    g = x.astype(np.float64) * ss[..., 0].astype(np.float64)[..., None, None] + ss[..., 1].astype(np.float64)[..., None, None]
    pooled = {"x": g.mean(axis=3).transpose(0, 2, 1), "y": g.mean(axis=2).transpose(0, 2, 1)}     # [B, H, C], [B, W, C]
    ref = {}
    for tag in ("x", "y"):
        uu = reducer64(pooled[tag], w, "chain" + tag)                                            # [B, Out, n]
        qk = np.einsum("mo,bon->bmn", w["chain%s.to_qk.weight" % tag].astype(np.float64), uu)
        ref["u" + tag], ref["k" + tag] = uu, lrk64(qk, heads, DK, invf)
        ref["k%s@oracle" % tag] = lrk64(qk, heads, DK, invf, "oracle")       # what chain_oracle is measured against
    return dict(c, x=x, ss=ss, w=w, invf=invf, ref=ref)


def chain_oracle():
    """The float32 oracle on the chain's inputs, in the reference's order (Linear, then the mean over the other axis):
    lns_oracle._pooling_reducer on the normalised field, then lns_oracle._low_rank_kernel -> {ux, uy [B, Out, n], kx, ky}."""
    import lns_oracle
    c = chain_set()
    g = (c["x"] * c["ss"][..., 0][..., None, None] + c["ss"][..., 1][..., None, None]).astype(np.float32)
    out = {}
    for tag, field in (("x", g), ("y", np.ascontiguousarray(g.transpose(0, 1, 3, 2)))):
        sd = dict(c["w"])
        sd["chain%s.pos_emb.inv_freq" % tag] = c["invf"]
        u = lns_oracle._pooling_reducer(sd, "chain" + tag, field)                                # [B, n, Out]
        out["u" + tag] = np.ascontiguousarray(u.transpose(0, 2, 1))
        out["k" + tag] = lns_oracle._low_rank_kernel(sd, "chain" + tag, u, c["heads"])
    return out

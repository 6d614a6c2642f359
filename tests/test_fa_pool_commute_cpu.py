"""CPU: the identity behind FABlock2D's pooling of its normalised input (DESIGN.md "FABlock2D: pooling in front of to_in"),
and what the change must leave alone.

The reference computes u_x = mean_W(Linear_x(to_in(in_norm(u)))): in_norm is affine per (sample, channel), to_in (1x1 conv)
and Linear_x carry no bias and act on channels only, the mean runs over a spatial axis.  So
mean_W(Linear_x(to_in(s u + t))) = (W_x W_toin)(s mean_W(u) + t), which is what the engine evaluates: the pooling kernel
gives s mean(u) + t and the reducer's first matrix is W_x W_toin, composed by fold_conv_1x1 (csrc/lns_fold.h, checked under
sanitizers by tests/test_fold_cpu.py; the composition adds no host code beyond that call)."""
import numpy as np
import pytest

from helpers import manifest, synthetic_state_dict

SHAPES = [(2, 64, 16, 16), (2, 64, 15, 30), (3, 32, 7, 15)]


def _rel(a, b):
    return float(np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel()))


def _both_orders(dt, B, C, H, W, seed):
    r = np.random.default_rng(seed)
    u = (r.standard_normal((B, C, H, W)) + r.uniform(-2, 2, (1, C, 1, 1))).astype(dt)
    s = (r.uniform(0.3, 2.0, (B, C, 1, 1)) * r.choice([-1.0, 1.0], (B, C, 1, 1))).astype(dt)
    t = r.uniform(-1, 1, (B, C, 1, 1)).astype(dt)
    w_toin = (r.standard_normal((C, C)) / np.sqrt(C)).astype(dt)
    w_ax = [(r.standard_normal((C, C)) / np.sqrt(C)).astype(dt) for _ in range(2)]
    out = []
    for ax, w in zip((3, 2), w_ax):                       # u_x: mean over W; u_y: mean over H
        v = np.einsum("oc,bchw->bohw", w_toin, u * s + t)                 # reference order
        ref = np.einsum("oc,bchw->bohw", w, v).mean(axis=ax, dtype=dt)
        wc = (w.astype(np.float64) @ w_toin.astype(np.float64)).astype(dt)     # composed in double, rounded once
        pooled = u.mean(axis=ax, dtype=dt) * s[..., 0] + t[..., 0]        # [B,C,n]
        out.append((ref, np.einsum("oc,bcn->bon", wc, pooled)))
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pooling_commutes_with_to_in_and_the_first_linear(shape):
    for (r64, c64), (r32, c32) in zip(_both_orders(np.float64, *shape, seed=1), _both_orders(np.float32, *shape, seed=1)):
        e64, e32 = _rel(c64, r64), _rel(c32, r32)
        print("%s: float64 %.2e, fp32 %.2e" % (shape, e64, e32))
        assert e64 <= 1e-12, e64
        assert e32 <= 1e-6, e32
        assert _rel(c32.astype(np.float64), r64) <= 1e-6


def test_parameter_table_is_unchanged_and_the_engine_builds():
    """to_in.0.weight stays a parameter (it has no conv pack any more); the table equals the reference's state_dict.  Loading
    weights composes the reducer matrices on the host and then needs a device: without one the ONLY acceptable failure is the
    HIP runtime saying so."""
    import torch
    from lns_amd import _lib, config, engine
    args = config.preset("ns2d_mini")
    eng = engine.Engine(engine.make_config(args, ae_prefix="vq_ae.", prop_prefix="propagator."))
    got = eng.param_shapes()
    ref = {k: tuple(v) for k, v in manifest()["ns2d_mini"].items()}
    assert {k: tuple(v) for k, v in got.items()} == ref
    toin = [k for k in got if k.endswith(".to_in.0.weight")]
    assert toin and all(len(got[k]) == 4 and got[k][0] == got[k][1] for k in toin), toin
    for k in toin:
        blk = k[: -len(".to_in.0.weight")]
        assert got[blk + ".to_x.0.to_in.weight"] == got[k][:2] and got[blk + ".to_y.1.to_in.weight"] == got[k][:2]
    sd = synthetic_state_dict(ref, 1)
    if torch.cuda.is_available():
        eng.load_weights(sd, 0)
        return
    with pytest.raises(_lib.LnsError) as ei:
        eng.load_weights(sd, 0)
    msg = str(ei.value)
    assert "lns_finalize_weights" in msg and "hip" in msg and "failed" in msg, msg

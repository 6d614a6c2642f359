"""GPU: the observation loss of the latent fit (lns_loss_obs_mse, csrc/latent_fit.inc) against its two statements in
tests/latent_fit_reference.py: the gradients equal the unfused float32 torch statement bit for bit (one subtraction, one
multiplication by a coefficient rounded once from double), steps that are not observed are exact zeros over a NaN-filled
buffer, `per` and `loss` stay within max(2e-7, 3 x torch's own float32 error) of float64, and pointers 4 bytes off a
16-byte boundary give the same bits.

Sizes: n = 1 (a block with one working lane), 63 (less than a wave), 256 (every thread exactly one element), 4097 (an odd
tail after 16 full passes), 18432 (c = 64 on 16x18: the largest latent of the presets); B = 1 and 3; T = 5."""
import numpy as np
import pytest
import torch

import latent_fit_reference as lf

pytestmark = pytest.mark.gpu

T = 5
TABLES = [([0], [1.0]), ([4], [0.25]), ([1, 3], [0.0, 0.5]), ([0, 1, 2, 3, 4], [1.0, 0.0, 0.5, 2.0, 1.0])]
KINDS = {"normal": (1.0, 0.0), "tiny": (1e-12, 0.0), "huge": (1e12, 0.0), "offset": (1e-2, 1e3)}
LAM = 0.3


def _need_gpu():
    assert torch.cuda.is_available(), "GPU test selected but no GPU is visible"


def _inputs(B, n, n_obs, kind, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 7 * n + B + n_obs)
    scale, shift = KINDS[kind]
    mk = lambda *s: (torch.randn(*s, generator=g, dtype=torch.float64) * scale + shift).to(torch.float32)      # noqa: E731
    return mk(B, T, n), mk(B, n_obs, n), mk(B, n), mk(B, n)


def _off(t):
    """the same values at a data pointer 4 bytes past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _rel(a, ref):
    a, ref = a.double().cpu(), ref.double().cpu()
    return ((a - ref).abs() / ref.abs().clamp_min(1e-300)).max().item() if ref.numel() else 0.0


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", [1, 63, 256, 4097, 18432])
def test_obs_loss_matches_both_statements(n, B):
    _need_gpu()
    from lns_amd import engine
    for steps, weights in TABLES:
        for bg in (False, True):
            zp, ob, z0, zb = _inputs(B, n, len(steps), "normal")
            d = [t.cuda() for t in (zp, ob, z0, zb)]
            grad = torch.full((B, T, n), float("nan"), device="cuda")
            kw = dict(z0=d[2], z_background=d[3], background=LAM) if bg else {}
            loss, per, g, gbg = engine.obs_loss(d[0], d[1], steps, weights, grad_out=grad, **kw)
            assert g is grad
            rg, rbg = lf.obs_grad_fp32(zp, ob, steps, weights, z0 if bg else None, zb if bg else None, LAM)
            assert torch.equal(g.cpu(), rg), (steps, bg)
            for t in range(T):
                if t not in steps:
                    assert (g[:, t] == 0).all()                       # exact zeros over the NaN fill
            if bg:
                assert torch.equal(gbg.cpu(), rbg)
            else:
                assert gbg is None
            l64, p64 = lf.obs_loss(zp.double(), ob.double(), steps, weights, z0.double(), zb.double() if bg else None, LAM)
            l32, p32 = lf.obs_loss(zp, ob, steps, weights, z0, zb if bg else None, LAM)
            for ours, r64, r32, what in ((per, p64, p32, "per"), (loss, l64, l32, "loss")):
                own, err = _rel(r32, r64), _rel(ours, r64)
                assert err <= max(2e-7, 3 * own), (what, steps, bg, err, own)
            # pointers 4 bytes off: the same bits
            o = [_off(t) for t in d]
            kw2 = dict(z0=o[2], z_background=o[3], background=LAM) if bg else {}
            loss2, per2, g2, gbg2 = engine.obs_loss(o[0], o[1], steps, weights, grad_out=_off(grad), **kw2)
            assert torch.equal(loss2, loss) and torch.equal(per2, per) and torch.equal(g2, g)
            assert gbg2 is None or torch.equal(gbg2, gbg)


@pytest.mark.parametrize("kind", ["tiny", "huge", "offset"])
def test_obs_loss_scales(kind):
    """1e-12 x, 1e12 x and 1e3 + 1e-2 x inputs: squares and sums in double neither flush nor overflow nor cancel."""
    _need_gpu()
    from lns_amd import engine
    for n, B in ((63, 3), (4097, 1)):
        steps, weights = TABLES[2]
        zp, ob, z0, zb = _inputs(B, n, len(steps), kind, seed=1)
        d = [t.cuda() for t in (zp, ob, z0, zb)]
        loss, per, g, gbg = engine.obs_loss(d[0], d[1], steps, weights, z0=d[2], z_background=d[3], background=LAM)
        rg, rbg = lf.obs_grad_fp32(zp, ob, steps, weights, z0, zb, LAM)
        assert torch.equal(g.cpu(), rg) and torch.equal(gbg.cpu(), rbg)
        l64, p64 = lf.obs_loss(zp.double(), ob.double(), steps, weights, z0.double(), zb.double(), LAM)
        l32, p32 = lf.obs_loss(zp, ob, steps, weights, z0, zb, LAM)
        assert np.isfinite(loss.cpu().numpy()).all() and (per.cpu() > 0).all()
        for ours, r64, r32, what in ((per, p64, p32, "per"), (loss, l64, l32, "loss")):
            own, err = _rel(r32, r64), _rel(ours, r64)
            print(kind, n, what, "ours %.3g torch fp32 %.3g" % (err, own))
            assert err <= max(2e-7, 3 * own), (kind, what, err, own)

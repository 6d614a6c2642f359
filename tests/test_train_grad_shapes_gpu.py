"""GPU: gradients of the training rollout against the float64 autograd reference (tests/train_reference.py) at the shapes
the recorded fixtures miss -- B up to 300, T = 1, the NS2d propagator on 8x8 and 16x16 circular latents, D = 32 / 96,
planes on either side of the 64-pixel chunk of both weight-gradient forms, wraps nearly as long as the axis, a one-row
plane -- with EVERY element of every propagator gradient, grad_z_in, z_pred and the loss compared, for both weight-gradient
forms (option "train_wgrad" 0 and 1).

The drop-in's training path takes h and w from z_in (dropin._LatentRolloutFn -> Engine.train_forward reads z_in.shape), so
one model per engine serves every size of its row; the autoencoder around the propagator only has to exist.

Tolerance, per tensor and in two measures (rel-L2, and max |engine - f64| / max |f64| so that one wrong element comparable
to the largest fails even in a large tensor): max(GRAD_TOL, 3 x own), `own` = the same reference run in float32 on the CPU
against its float64 run, in the same measure -- the rule of tests/test_gpu_parity.py.  Loss 2e-6 relative + 1e-7 and z_pred
2e-5 as in the fixture test.  tests/test_train_reference_cpu.py holds 3 x own <= 1e-3 for every case on the CPU.

No case of the grid is refused by lns_create or by the training calls (1x130 and 2x2 included)."""
import pytest
import torch

import train_reference as tr

pytestmark = pytest.mark.gpu


def _need_gpu():
    assert torch.cuda.is_available(), "GPU test selected but no GPU is visible"


@pytest.mark.parametrize("form", tr.FORMS)
@pytest.mark.parametrize("case", tr.CASES, ids=tr.case_id)
def test_gradients_match_float64_reference(case, form):
    _need_gpu()
    rows, dloss, loss, ezp = tr.compare(case, form)
    worst = max(rows, key=lambda r: max(r[1] / r[2], r[3] / r[4]))
    print("%s form %d: loss %.6f (off %.2e) z_pred %.2e worst %s rel-L2 %.2e/%.2e rel-max %.2e/%.2e (own %.2e %.2e)"
          % ((tr.case_id(case), form, loss, dloss, ezp) + worst))
    assert dloss <= 2e-6 * abs(loss) + 1e-7, (dloss, loss)
    assert ezp < 2e-5, ezp
    for k, e2, b2, em, bm, o2, om in rows:
        assert e2 <= b2, (k, "rel-L2", e2, b2, o2)
        assert em <= bm, (k, "rel-max", em, bm, om)

"""Fitting the initial latent to observed latents by Adam and by Gauss-Newton, on one box and in one process (synthetic
latents, B = 32, T = 4 rollout steps, observations at steps [1, 3]), for the four shapes of tools/latent_fit_time.py:
  (a) lns_amd.fit.LatentFit.run, 40 iterations (lns_fit_step: forward, observation loss, state-only adjoint, Adam)
  (b) lns_amd.fit.LatentFit.run_gauss_newton, 3 outer x 8 CG (lns_fit_gn_step: forward, loss, adjoint, then per CG step one
      tangent-linear rollout, one state-only adjoint and the per-sample double-precision CG kernels)
Warm-up, then blocks of ONE whole fit per arm with one synchronisation before and after, the arms interleaved block by block;
per arm the median wall time of a fit with its min / max, the worst-sample and median final loss over loss[0], and the kernel
launches of one whole fit as torch.profiler counts them (null where the profiler gives no kernel events), from which the
launches per outer iteration of (b) follow.

    python tools/latent_fit_gn_time.py [--blocks 5] [--warmup 1] [--out profiles/latent_fit_gn_time.json]

What a run does not show: both arms include their per-call set-up (clones, zeroed moments, output tensors) and (b) one extra
forward and observation loss for its last loss row; the observations are random latents, not a trajectory of the model, so the
losses say how far each optimiser gets on an inconsistent problem in its budget, not how well a twin is recovered (that is
profiles/latent_fit_gn_parity.json); wall time of a fit, not GPU kernel time; nothing here is a gate.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from lns_amd import filler, fit  # noqa: E402
import latent_fit_time  # noqa: E402
import train_time  # noqa: E402

T, STEPS, B = latent_fit_time.T, latent_fit_time.STEPS, latent_fit_time.B
ADAM_ITERS, OUTER, CG_ITERS = 40, 3, 8


def arms_for(preset, dev):
    args, model = train_time.build(preset, dev)
    model._eng.set_option("train_wgrad", 0)
    c, h, w = model._eng.latent_shape()
    cond = model._conditional
    z_start = torch.from_numpy(filler.normal("z_in", (B, c, h, w), 11) * 0.5).to(dev)
    obs = torch.from_numpy(filler.normal("obs", (B, len(STEPS), c, h, w), 11) * 0.5).to(dev)
    prm = torch.from_numpy(filler.uniform01("param", B, 11).astype("float32")).to(dev) if cond else None
    fitter = fit.LatentFit(model, lr_state=latent_fit_time.LR, fit_param=False)
    last = {}

    def adam_arm():
        last["a_adam_40"] = fitter.run(z_start, obs, STEPS, param=prm, iters=ADAM_ITERS).loss

    def gn_arm():
        last["b_gauss_newton_3x8"] = fitter.run_gauss_newton(z_start, obs, STEPS, param=prm, outer=OUTER, cg_iters=CG_ITERS).loss
    return {"a_adam_40": adam_arm, "b_gauss_newton_3x8": gn_arm}, last, (c, h, w)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rec = {"B": B, "T": T, "obs_steps": STEPS, "blocks": a.blocks, "adam_iters": ADAM_ITERS, "outer": OUTER, "cg_iters": CG_ITERS,
           "device": torch.cuda.get_device_name(0), "shapes": {}}
    for preset, _ in train_time.SHAPES:
        arms, last, latent = arms_for(preset, dev)
        for run in arms.values():
            for _ in range(a.warmup):
                run()
        torch.cuda.synchronize()
        times = {k: [] for k in arms}
        for _ in range(a.blocks):
            for k, run in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run()
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) * 1e3)
        row = {"latent": list(latent)}
        for k, v in times.items():
            loss = last[k].double().cpu()
            # (a)'s last row is the loss BEFORE its last update, (b)'s the loss of the returned state
            ratio = loss[-1] / loss[0]
            row[k] = {"ms_per_fit_median": statistics.median(v), "min": min(v), "max": max(v),
                      "final_over_first_loss_worst": float(ratio.max()), "final_over_first_loss_median": float(ratio.median()),
                      "final_loss_mean": float(loss[-1].mean()), "first_loss_mean": float(loss[0].mean()),
                      "launches_per_fit": latent_fit_time.launches(lambda n, run=arms[k]: run())}
        n_fit = row["b_gauss_newton_3x8"]["launches_per_fit"]
        row["b_launches_per_outer_iteration"] = n_fit / OUTER if n_fit else None     # (includes a third of the closing forward + loss)
        row["b_over_a_time"] = row["b_gauss_newton_3x8"]["ms_per_fit_median"] / row["a_adam_40"]["ms_per_fit_median"]
        row["a_block_spread_max_over_min"] = row["a_adam_40"]["max"] / row["a_adam_40"]["min"]
        rec["shapes"][preset] = row
        print(preset, json.dumps(row))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

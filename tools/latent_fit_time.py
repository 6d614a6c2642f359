"""Fitting the initial latent to observed latents, two ways, on one box and in one process (synthetic latents, B = 32,
T = 4 rollout steps, observations at steps [1, 3]), for the four shapes of tools/train_time.py:
  (a0) / (a1) what existed before lns_fit_step: z0.requires_grad_(); model(z0, ...) through the drop-in's autograd rollout
              (every propagator gradient is computed and thrown away), a torch MSE on the observed steps, torch.optim.Adam([z0]);
              engine option "train_wgrad" 0 / 1
  (b)         lns_amd.fit.LatentFit.run (lns_fit_step: forward, observation loss, state-only adjoint, Adam in one C call)
Warm-up, then blocks of 10 iterations with one synchronisation before and after each block, the arms interleaved block by
block; per arm the median block time and its min / max, (a) / (b) beside (a)'s own block spread, and the kernel launches of one
iteration of each arm as torch.profiler counts them (null where the profiler gives no kernel events).

    python tools/latent_fit_time.py [--blocks 5] [--block 10] [--warmup 1] [--out profiles/latent_fit_time.json]

What a run does not show: (b)'s block includes LatentFit.run's per-call set-up (clones of z0, zeroed moments, the loss tensor),
(a)'s does not; the param fit is not timed (arm (a) had no gradient with respect to param to compare with); wall time of a
block, not GPU kernel time -- the share of the skipped weight-gradient kernels is in DESIGN.md section 6f, from a kernel trace.
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
import train_time  # noqa: E402

T, STEPS, B = 4, [1, 3], 32
LR = 2e-3


def arms_for(preset, dev):
    args, model = train_time.build(preset, dev)
    c, h, w = model._eng.latent_shape()
    cond = model._conditional
    z_start = torch.from_numpy(filler.normal("z_in", (B, c, h, w), 11) * 0.5).to(dev)
    obs = torch.from_numpy(filler.normal("obs", (B, len(STEPS), c, h, w), 11) * 0.5).to(dev)
    prm = torch.from_numpy(filler.uniform01("param", B, 11).astype("float32")).to(dev) if cond else None
    dummy = torch.empty((B, T, c, h, w), device=dev)

    def loss_fn(pred, _):
        return ((pred[:, STEPS] - obs) ** 2).flatten(2).mean(2).sum()

    def autograd_arm(form):
        z0 = z_start.clone()[:, None].requires_grad_(True)
        opt = torch.optim.Adam([z0], lr=LR)

        def run(n):
            model._eng.set_option("train_wgrad", form)
            for _ in range(n):
                opt.zero_grad()
                loss = model(z0, dummy, prm, loss_fn) if cond else model(z0, dummy, loss_fn)
                loss.backward()
                opt.step()
        return run
    fitter = fit.LatentFit(model, lr_state=LR, fit_param=False)

    def fit_arm(n):
        model._eng.set_option("train_wgrad", 0)
        fitter.run(z_start, obs, STEPS, param=prm, iters=n)
    return {"a0_autograd_tile": autograd_arm(0), "a1_autograd_split": autograd_arm(1), "b_latent_fit": fit_arm}, (c, h, w)


def launches(run):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            run(1)
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
                and "memset" not in e.name.lower())
        return n or None
    except Exception as ex:  # noqa: BLE001
        print("launch count unavailable: %s" % ex)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--block", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rec = {"B": B, "T": T, "obs_steps": STEPS, "block": a.block, "blocks": a.blocks, "device": torch.cuda.get_device_name(0), "shapes": {}}
    for preset, _ in train_time.SHAPES:
        arms, latent = arms_for(preset, dev)
        for run in arms.values():
            for _ in range(a.warmup):
                run(a.block)
        torch.cuda.synchronize()
        times = {k: [] for k in arms}
        for _ in range(a.blocks):
            for k, run in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(a.block)
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) / a.block * 1e3)
        row = {"latent": list(latent)}
        for k, v in times.items():
            row[k] = {"ms_per_iter_median": statistics.median(v), "min": min(v), "max": max(v), "launches_per_iter": launches(arms[k])}
        for k in ("a0_autograd_tile", "a1_autograd_split"):
            row[k + "_over_b"] = row[k]["ms_per_iter_median"] / row["b_latent_fit"]["ms_per_iter_median"]
            row[k + "_block_spread_max_over_min"] = row[k]["max"] / row[k]["min"]
        rec["shapes"][preset] = row
        print(preset, json.dumps(row))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

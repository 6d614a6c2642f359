"""Stage-2 training step, four ways (six with --clip), on one box and in one process (synthetic latents, B = 32):
  (a) autograd      : model(z_in, z_out[, param], F.smooth_l1_loss); loss.backward(); torch.optim.Adam.step()
  (b) lns Adam      : the same with lns_amd.optim.Adam (one-launch multi-tensor kernel)
  (c) trainer       : lns_amd.train.Stage2Trainer.step (lns_train_step: forward, loss, backward and Adam in one C call)
  (d) trainer_split : the same with wgrad="split" (engine option "train_wgrad" = 1: the batch-parallel weight gradient)
  (e) trainer_clip  : --clip only: Stage2Trainer(max_grad_norm=1.0) (lns_train_step_clip: + norm and clipped update), in the
                      weight-gradient form --clip-wgrad names (default split); its yardstick is (c) / (d) of the same form
  (f) unfused_clip  : --clip only: what a user wrote before: step(update=False); torch.nn.utils.clip_grad_norm_(params, 1.0);
                      lns_amd.optim.Adam.step(), same form
for the reference's shipped training shapes: ns2d_64 (T = 2), sw_half_periodic (T = 5), twophase_cond (T = 5), and
ns2d_128 (T = 2).  Warm-up, then blocks of 10 steps with one synchronisation before and after each block, the arms
interleaved block by block; per arm the median block time, its min / max, steps/s and trajectory-steps/s (B * T / time).

    python tools/train_time.py [--blocks 5] [--block 10] [--warmup 5] [--out profiles/train_step_time_wgrad.json]
    python tools/train_time.py --clip --out profiles/train_step_time_clip.json
    python tools/train_time.py --only-trainer --preset ns2d_64 --blocks 3      # the runs to put under rocprofv3 --kernel-trace --stats,
    python tools/train_time.py --only-trainer-split --preset ns2d_64 --blocks 3  # one per arm
    python tools/train_time.py --merge-stats ns2d_64:25=out/..._kernel_stats.csv trainer_split/ns2d_64:25=... --out profiles/train_step_time_wgrad.json
The last form ([ARM/]PRESET:STEPS=CSV, ARM = trainer by default, STEPS = warm-up + timed steps of the profiled run) adds, per
preset and arm, the GPU kernel time of one step (sum of the kernel-stats totals / steps run), its share of the measured step
time, the share of the weight-gradient kernels in it and the per-kernel totals (largest first) to an existing record.
(profiles/train_step_time.json is the record of the three-arm form of this tool, before the split arm existed.)
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lns_amd import config, dropin, filler, optim, train  # noqa: E402

SHAPES = (("ns2d_64", 2), ("sw_half_periodic", 5), ("twophase_cond", 5), ("ns2d_128", 2))
B = 32
Z_SCALE = 0.5          # as the gradient fixtures (tools/make_golden.py grads)
LR = 5e-4


def build(preset, dev):
    args = config.preset(preset)
    model = dropin.build_dynamics(args)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(v) for k, v in filler.synthetic_state_dict(shapes, 1).items()})
    model = model.to(dev)
    for p in model._ae.parameters():
        p.requires_grad_(False)
    return args, model


def arms_for(preset, T, dev, only=None, clip_wgrad=None):
    args, probe = build(preset, dev)
    c, h, w = probe._eng.latent_shape()
    del probe
    z_in = torch.from_numpy(filler.normal("z_in", (B, 1, c, h, w), 5) * np.float32(Z_SCALE)).to(dev)
    z_out = torch.from_numpy(filler.normal("z_out", (B, T, c, h, w), 5) * np.float32(Z_SCALE)).to(dev)
    prm = (torch.from_numpy(filler.uniform01("param", B, 5).astype(np.float32)).to(dev),) if args.family == "twophase_cond" else ()

    def autograd_arm(opt_cls):
        _, model = build(preset, dev)
        opt = opt_cls(model.propagator.parameters(), lr=LR)

        def step():
            opt.zero_grad()
            loss = model(z_in, z_out, *prm, F.smooth_l1_loss)
            loss.backward()
            opt.step()
            return loss
        return step

    def trainer_arm(wgrad):
        _, model = build(preset, dev)            # (its own model, hence its own engine: the option is per engine)
        tr = train.Stage2Trainer(model, lr=LR, wgrad=wgrad)
        return lambda: tr.step(z_in, z_out, *prm)
    def clip_arm():
        _, model = build(preset, dev)
        tr = train.Stage2Trainer(model, lr=LR, wgrad=clip_wgrad, max_grad_norm=1.0)
        return lambda: tr.step(z_in, z_out, *prm)

    def unfused_clip_arm():
        _, model = build(preset, dev)
        tr = train.Stage2Trainer(model, lr=LR, wgrad=clip_wgrad)
        params = list(model.propagator.parameters())

        def step():
            loss = tr.step(z_in, z_out, *prm, update=False)
            torch.nn.utils.clip_grad_norm_(params, 1.0)
            tr.optimizer.step()
            return loss
        return step
    makers = {"autograd": lambda: autograd_arm(torch.optim.Adam), "lns_adam": lambda: autograd_arm(optim.Adam),
              "trainer": lambda: trainer_arm("tile"), "trainer_split": lambda: trainer_arm("split")}
    if clip_wgrad:
        makers.update(trainer_clip=clip_arm, unfused_clip=unfused_clip_arm)
    return {k: mk() for k, mk in makers.items() if only is None or k in only}, (c, h, w)


def block_ms(step, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        loss = step()
    torch.cuda.synchronize()
    del loss
    return (time.perf_counter() - t0) * 1e3


def measure(preset, T, a, dev):
    only = ("trainer",) if a.only_trainer else ("trainer_split",) if a.only_trainer_split else None
    arms, latent = arms_for(preset, T, dev, only, a.clip_wgrad if a.clip else None)
    for step in arms.values():
        for _ in range(a.warmup):
            step()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(a.blocks):
        for k, step in arms.items():
            times[k].append(block_ms(step, a.block))
    rec = dict(preset=preset, B=B, T=T, latent=list(latent), block_steps=a.block, blocks=a.blocks, steps_timed_per_arm=a.block * a.blocks)
    for k, v in times.items():
        med = statistics.median(v) / a.block
        rec[k] = dict(step_ms_median=round(med, 4), step_ms_min=round(min(v) / a.block, 4), step_ms_max=round(max(v) / a.block, 4),
                      steps_per_s=round(1e3 / med, 2), trajectory_steps_per_s=round(B * T * 1e3 / med, 1),
                      block_ms=[round(x, 3) for x in v])
    if "autograd" in rec:
        base = rec["autograd"]
        rec["speedup_trainer_over_autograd"] = round(base["step_ms_median"] / rec["trainer"]["step_ms_median"], 4)
        rec["speedup_lns_adam_over_autograd"] = round(base["step_ms_median"] / rec["lns_adam"]["step_ms_median"], 4)
        rec["autograd_spread_max_over_min"] = round(base["step_ms_max"] / base["step_ms_min"], 4)
        rec["trainer_within_autograd_spread"] = bool(base["step_ms_min"] <= rec["trainer"]["step_ms_median"] <= base["step_ms_max"])
    if "trainer" in rec and "trainer_split" in rec:
        # the yardstick of the split arm is the trainer arm of the same run (option 0): a gain only counts when the split
        # arm's median is below the FASTEST block of that arm
        tile, split = rec["trainer"], rec["trainer_split"]
        rec["speedup_split_over_trainer"] = round(tile["step_ms_median"] / split["step_ms_median"], 4)
        rec["trainer_spread_max_over_min"] = round(tile["step_ms_max"] / tile["step_ms_min"], 4)
        rec["split_median_below_trainer_min"] = bool(split["step_ms_median"] < tile["step_ms_min"])
    if "trainer_clip" in rec:
        # the yardstick of the clipped arm is the unclipped trainer of the same form in the same run; a cost only counts when
        # the clipped arm's median lies outside that arm's block spread
        yard_name = "trainer_split" if a.clip_wgrad == "split" else "trainer"
        yard, clip, unf = rec[yard_name], rec["trainer_clip"], rec["unfused_clip"]
        rec["clip_wgrad"] = a.clip_wgrad
        rec["clip_yardstick_arm"] = yard_name
        rec["clip_median_within_yardstick_spread"] = bool(yard["step_ms_min"] <= clip["step_ms_median"] <= yard["step_ms_max"])
        rec["clip_over_yardstick"] = round(clip["step_ms_median"] / yard["step_ms_median"], 4)
        rec["yardstick_spread_max_over_min"] = round(yard["step_ms_max"] / yard["step_ms_min"], 4)
        rec["speedup_clip_over_unfused"] = round(unf["step_ms_median"] / clip["step_ms_median"], 4)
        rec["clip_median_below_unfused_min"] = bool(clip["step_ms_median"] < unf["step_ms_min"])
    return rec


def merge_stats(a):
    with open(a.out) as f:
        doc = json.load(f)
    for item in a.merge_stats:
        spec, path = item.split("=", 1)
        preset, _, steps = spec.partition(":")
        arm, _, preset = preset.rpartition("/")
        arm = arm or "trainer"
        with open(path) as f:
            rows = list(csv.DictReader(f))
        total_ns = sum(float(r["TotalDurationNs"]) for r in rows)
        calls = sum(int(r["Calls"]) for r in rows)
        rec = next(r for r in doc["shapes"] if r["preset"] == preset)
        n = int(steps)
        gpu_ms = total_ns / 1e6 / n
        out = rec[arm]
        out["gpu_kernel_ms_per_step"] = round(gpu_ms, 4)
        out["kernel_launches_per_step"] = round(calls / n, 1)
        out["gpu_kernel_share_of_step"] = round(gpu_ms / out["step_ms_median"], 4)
        out["gpu_kernel_time_source"] = "rocprofv3 --kernel-trace --stats over %d steps (warm-up included), a run of its own" % n
        wgrad_ns = sum(float(r["TotalDurationNs"]) for r in rows if "wgrad" in r["Name"])
        out["wgrad_share_of_kernel_time"] = round(wgrad_ns / total_ns, 4)
        top = sorted(rows, key=lambda r: -float(r["TotalDurationNs"]))[:8]
        out["kernels_ms_per_step"] = [dict(name=r["Name"].split("(")[0][:96], ms=round(float(r["TotalDurationNs"]) / 1e6 / n, 4),
                                           calls_per_step=round(int(r["Calls"]) / n, 1),
                                           share=round(float(r["TotalDurationNs"]) / total_ns, 4)) for r in top]
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default=None, help="one of the four shapes (default: all)")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--block", type=int, default=10, help="steps per synchronised block")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only-trainer", action="store_true")
    ap.add_argument("--only-trainer-split", action="store_true")
    ap.add_argument("--clip", action="store_true", help="add the clipped trainer and the unfused clip sequence (arms e, f)")
    ap.add_argument("--clip-wgrad", choices=("tile", "split"), default="split")
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge-stats", nargs="*", default=None, metavar="PRESET:STEPS=CSV")
    a = ap.parse_args()
    if a.merge_stats is not None:
        return merge_stats(a)
    dev = torch.device("cuda", 0)
    shapes = [s for s in SHAPES if a.preset in (None, s[0])]
    doc = dict(tool="train_time", device=torch.cuda.get_device_name(dev), torch=torch.__version__, lr=LR, z_scale=Z_SCALE,
               shapes=[measure(p, T, a, dev) for p, T in shapes])
    print(json.dumps(doc))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()

"""Validation step with per-pixel time maps, four ways, on one box and in one process (default options, arms interleaved):
  (a) Engine.rollout_eval                          -- the streaming validation without maps: the yardstick
  (b) Engine.rollout_eval_maps, maps over every step
  (c) Engine.rollout_eval_maps, over every 8th step
  (d) what exists without the call: Engine.rollout -> [B,T,C,Ly,Lx] in HBM -> metrics.relative_l2 -> the same seven maps in
      torch on the stored tensor (mean / var / covariance / mse / amax over the time axis), 8 trajectories at a time
Warm-up, then `blocks` synchronised blocks of `calls` calls per arm; the figure of an arm is the median over its blocks of
(block time / calls), (a)'s spread is (max - min) / median over its blocks.  Peak torch allocation of each arm above what
is resident before it.  The result is merged into a JSON file under the key "T<rollout>".

    python tools/eval_maps_time.py [--preset ns2d_128] [--batch 64] [--rollout 64] [--out profiles/rollout_eval_maps_time.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d out -- python tools/eval_maps_time.py --only-b 3    # arm (b) alone
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lns_amd import config, dropin, filler, metrics  # noqa: E402
from eval_time import norm_for  # noqa: E402


def torch_maps(p, q):
    """p, q [b, T, C, H, W] denormalised -> [b, C, 7, H, W] with torch's reductions over the time axis (metrics.TIME_MAPS)."""
    n = p.shape[1]
    mp, mq = p.mean(1), q.mean(1)
    vp, vq = p.var(1, unbiased=True), q.var(1, unbiased=True)
    cov = ((p - mp.unsqueeze(1)) * (q - mq.unsqueeze(1))).sum(1) / max(n - 1, 1)
    e = p - q
    return torch.stack([mp, mq, vp, vq, cov, (e * e).mean(1), e.abs().amax(1)], 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="ns2d_128")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rollout", type=int, default=64)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only-b", type=int, default=0, help="run arm (b) this many times and nothing else (kernel traces)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_eval_maps_time.json"))
    a = ap.parse_args()
    B, T = a.batch, a.rollout
    if not torch.cuda.is_available():
        raise SystemExit("eval_maps_time needs a GPU: a time taken elsewhere says nothing")
    dev = torch.device("cuda", 0)
    args = config.preset(a.preset)
    C, H, W = args.in_channels, args.Ly, args.Lx
    model = dropin.build_dynamics(args)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(v) for k, v in filler.synthetic_state_dict(shapes, 1).items()})
    model = model.to(dev)
    x = torch.from_numpy(filler.normal("xeval", (B, C, H, W), 5)).to(dev)
    param = torch.from_numpy(filler.uniform01("peval", B, 5).astype("float32")).to(dev) if args.family == "twophase_cond" else None
    gen = torch.Generator(device=dev).manual_seed(11)
    y = torch.randn((B, T, C, H, W), generator=gen, device=dev)      # the stand-in ground truth
    norm = norm_for(args)
    eng = model._engine(x)
    eng.set_option("eval_max_steps", max(T, 1024))
    mean = torch.tensor(norm["mean"], device=dev).reshape(-1, 1, 1) if not isinstance(norm["mean"], float) else norm["mean"]
    std = torch.tensor(norm["std"], device=dev).reshape(-1, 1, 1) if not isinstance(norm["std"], float) else norm["std"]

    def arm_a():
        return eng.rollout_eval(x, y, param=param, **norm)[:2]

    def arm_b():
        return eng.rollout_eval_maps(x, y, param=param, **norm)

    def arm_c():
        return eng.rollout_eval_maps(x, y, param=param, map_steps=(0, 8), **norm)

    def arm_d():
        out = eng.rollout(x, T, param=param)
        f, s = metrics.relative_l2(out, y, **norm)
        maps = torch.empty((B, C, 7, H, W), device=dev)
        for b0 in range(0, B, 8):
            maps[b0:b0 + 8] = torch_maps(out[b0:b0 + 8] * std + mean, y[b0:b0 + 8] * std + mean)
        return f, s, maps

    if a.only_b:
        for _ in range(a.only_b):
            arm_b()
        torch.cuda.synchronize()
        return

    arms = {"a": arm_a, "b": arm_b, "c": arm_c, "d": arm_d}

    def block(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.calls):
            r = fn()
        torch.cuda.synchronize()
        del r
        return (time.perf_counter() - t0) * 1e3 / a.calls

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        r = fn()
        torch.cuda.synchronize()
        del r
        return torch.cuda.max_memory_allocated(dev) - base

    for _ in range(a.warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    ra, rb, rd = arm_a(), arm_b(), arm_d()
    torch.cuda.synchronize()
    same = all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(ra, (rb.frame, rb.seq)))
    # (d) is torch's fp32 reductions: agreement, not equality -- per map, the largest difference over the map's largest value
    d64 = rd[2].double()
    agree = float(((rb.maps.double() - d64).abs().amax((0, 1, 3, 4)) / d64.abs().amax((0, 1, 3, 4))).max())
    del ra, rb, rd
    times = {k: [] for k in arms}
    for _ in range(a.blocks):
        for k, fn in arms.items():
            times[k].append(block(fn))
    med = {k: statistics.median(v) for k, v in times.items()}
    peaks = {k: peak(fn) for k, fn in arms.items()}
    res = dict(
        tool="eval_maps_time", preset=a.preset, batch=B, rollout=T, blocks=a.blocks, calls_per_block=a.calls, warmup=a.warmup,
        device=torch.cuda.get_device_name(dev),
        ms_per_call={k: round(v, 3) for k, v in med.items()}, ms_per_call_blocks={k: [round(t, 3) for t in v] for k, v in times.items()},
        a_block_spread=round((max(times["a"]) - min(times["a"])) / med["a"], 4),
        b_over_a=round(med["b"] / med["a"], 4), c_over_a=round(med["c"] / med["a"], 4), d_over_b=round(med["d"] / med["b"], 4),
        peak_bytes_above_resident=peaks, rollout_tensor_bytes=B * T * C * H * W * 4, state_bytes=B * C * H * W * 52,
        frame_seq_bitwise_equal_a_b=bool(same), b_against_d_worst_relative_difference=agree)
    print(json.dumps(res))
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            doc = json.load(f)
    doc["T%d" % T] = res
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()

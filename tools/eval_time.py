"""Validation step, two ways, on one box and in one process:
  (a) two calls : Engine.rollout -> [B,T,C,Ly,Lx] in HBM -> metrics.relative_l2     (the path before lns_rollout_eval)
  (b) streaming : Engine.rollout_eval -- every decoded group is scored on its decode stream, the field is never stored
Warm-up, then the median of synchronised repetitions of each arm (interleaved a, b, a, b ...), the peak
torch.cuda.max_memory_allocated of each arm on its own, a bitwise comparison of the results, one JSON line.

    python tools/eval_time.py [--preset ns2d_128] [--batch 64] [--rollout 64] [--reps 7] [--warmup 2]
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
from lns_amd import config, dropin, filler, metrics  # noqa: E402

# per-family denormalisation (synthetic statistics; the kernel form is what matters: scalar / per-channel / two-phase)
SW_MEAN, SW_STD = [0.4, -0.2, 9.5, 0.15, -1.1], [2.1, 1.7, 0.6, 1.3, 0.9]


def norm_for(args):
    if args.family == "ns2d":
        return dict(mean=0.37, std=1.9)
    if args.family.startswith("sw"):
        return dict(mean=SW_MEAN[:args.in_channels], std=SW_STD[:args.in_channels])
    return metrics.twophase_spec(0.013, 0.21, 310.0, 180.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="ns2d_128")
    ap.add_argument("--batch", type=int, default=None, help="trajectories (default 64; 32 for twophase_cond)")
    ap.add_argument("--rollout", type=int, default=None, help="rollout length T (default 64; 128 for twophase_cond)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    B = a.batch or (32 if a.preset == "twophase_cond" else 64)
    T = a.rollout or (128 if a.preset == "twophase_cond" else 64)
    dev = torch.device("cuda", 0)
    args = config.preset(a.preset)
    model = dropin.build_dynamics(args)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(v) for k, v in filler.synthetic_state_dict(shapes, 1).items()})
    model = model.to(dev)
    x = torch.from_numpy(filler.normal("xeval", (B, args.in_channels, args.Ly, args.Lx), 5)).to(dev)
    param = torch.from_numpy(filler.uniform01("peval", B, 5).astype("float32")).to(dev) if args.family == "twophase_cond" else None
    gen = torch.Generator(device=dev).manual_seed(11)
    y = torch.randn((B, T, args.in_channels, args.Ly, args.Lx), generator=gen, device=dev)      # the stand-in ground truth
    norm = norm_for(args)
    eng = model._engine(x)
    eng.set_option("eval_max_steps", max(T, 1024))

    def two_call():
        out = eng.rollout(x, T, param=param)
        return metrics.relative_l2(out, y, **norm)

    def streaming():
        return eng.rollout_eval(x, y, param=param, **norm)[:2]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    def peak(fn):
        """Peak allocation of one call above what is resident before it (weights, x, y, cached workspaces)."""
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        r = fn()
        torch.cuda.synchronize()
        del r
        return torch.cuda.max_memory_allocated(dev), base

    for _ in range(a.warmup):
        ra, rb = two_call(), streaming()
    torch.cuda.synchronize()
    same = all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(ra, rb))
    del ra, rb
    ta, tb = [], []
    for _ in range(a.reps):
        ta.append(timed(two_call)[0])
        tb.append(timed(streaming)[0])
    pa, base_a = peak(two_call)
    pb, base_b = peak(streaming)
    ma, mb = statistics.median(ta), statistics.median(tb)
    field = B * T * args.in_channels * args.Ly * args.Lx * 4
    print(json.dumps(dict(
        tool="eval_time", preset=a.preset, batch=B, rollout=T, reps=a.reps, warmup=a.warmup, device=torch.cuda.get_device_name(dev),
        two_call_ms=round(ma, 3), streaming_ms=round(mb, 3), time_ratio_streaming_over_two_call=round(mb / ma, 4),
        two_call_ms_all=[round(v, 3) for v in ta], streaming_ms_all=[round(v, 3) for v in tb],
        two_call_peak_bytes=pa, streaming_peak_bytes=pb, peak_ratio_streaming_over_two_call=round(pb / pa, 4),
        resident_before_bytes=dict(two_call=base_a, streaming=base_b), rollout_tensor_bytes=field,
        peak_saving_bytes=pa - pb, results_bitwise_equal=bool(same))))


if __name__ == "__main__":
    main()

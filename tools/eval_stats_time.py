"""Validation step with field statistics, four ways, on one box and in one process (default options, arms interleaved):
  (a) Engine.rollout_eval                          -- the streaming validation without statistics: the yardstick
  (b) Engine.rollout_eval_stats, statistics and 64-bin histograms of every step
  (c) Engine.rollout_eval_stats, of every 8th step
  (d) what exists without the call: Engine.rollout -> [B,T,C,Ly,Lx] in HBM -> metrics.relative_l2 -> the same twelve
      statistics and the histograms in torch on the stored tensor, 16 steps at a time
Warm-up, then `blocks` synchronised blocks of `calls` calls per arm; the figure of an arm is the median over its blocks of
(block time / calls), (a)'s spread is (max - min) / median over its blocks.  Peak torch allocation of each arm above what
is resident before it.  The result is merged into a JSON file under the key "T<rollout>".

    python tools/eval_stats_time.py [--preset ns2d_128] [--batch 64] [--rollout 64] [--out profiles/rollout_eval_stats_time.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d out -- python tools/eval_stats_time.py --only-b 3    # arm (b) alone
    python tools/eval_stats_time.py --launches out/<host>/<pid>_kernel_trace.csv profiles/rollout_eval_stats_trace_launches.csv
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

NBINS, LO, HI = 64, -8.0, 8.0


def torch_stats(p, q, eps):
    """p, q [B, t, C, H, W] denormalised -> [B, t, C, 12] with torch's reductions (metrics.FIELD_STATS)."""
    d = (-2, -1)
    mp, mq = p.mean(d), q.mean(d)
    vp, vq = p.var(d, unbiased=False), q.var(d, unbiased=False)
    cov = ((p - mp[..., None, None]) * (q - mq[..., None, None])).mean(d)
    den = vp.sqrt() * vq.sqrt()
    corr = torch.where(den == 0, torch.zeros_like(den), cov / den)
    cos = (p * q).sum(d) / (((p * p).sum(d).sqrt() + eps) * ((q * q).sum(d).sqrt() + eps))
    gyp, gyq = p[..., 2:, :] - p[..., :-2, :], q[..., 2:, :] - q[..., :-2, :]
    gxp, gxq = p[..., :, 2:] - p[..., :, :-2], q[..., :, 2:] - q[..., :, :-2]
    gy = (((gyp - gyq) ** 2).sum(d) / (gyq * gyq).sum(d).clamp_min(eps)).sqrt()
    gx = (((gxp - gxq) ** 2).sum(d) / (gxq * gxq).sum(d).clamp_min(eps)).sqrt()
    return torch.stack([mp, mq, vp, vq, corr, cos, gy, gx, p.amin(d), p.amax(d), q.amin(d), q.amax(d)], -1)


def torch_hist(u, nbins, lo, hi):
    """u [B, t, C, H, W] -> int64 counts [B, t, C, nbins + 2] by the rule of include/lns.h (no NaN in u)."""
    scale = torch.tensor(nbins, dtype=torch.float32, device=u.device) / torch.tensor(hi - lo, dtype=torch.float32, device=u.device)
    k = 1 + ((u - lo) * scale).to(torch.int64).clamp(0, nbins - 1)
    k = torch.where(u < lo, torch.zeros_like(k), torch.where(u >= hi, torch.full_like(k, nbins + 1), k))
    planes = u.shape[0] * u.shape[1] * u.shape[2]
    off = torch.arange(planes, device=u.device).view(u.shape[:3] + (1, 1)) * (nbins + 2)
    return torch.bincount((k + off).reshape(-1), minlength=planes * (nbins + 2)).view(u.shape[:3] + (nbins + 2,))


def launches(trace_csv, out_csv, kernels=("field_stats_group_kernel", "metric_group_kernel")):
    """rocprofv3's <pid>_kernel_trace.csv -> one row per launch with the duration (End - Start, ns) of each of `kernels`."""
    import csv
    ns = {k: [] for k in kernels}
    with open(trace_csv) as f:
        for row in csv.DictReader(f):
            for k in kernels:
                if k in row["Kernel_Name"]:
                    ns[k].append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
    with open(out_csv, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["launch"] + ["%s_ns" % k for k in kernels])
        for i in range(max(len(v) for v in ns.values())):
            w.writerow([i] + [v[i] if i < len(v) else "" for v in ns.values()])
    for k, v in ns.items():
        print("%s: %d launches, median %.1f us (%.1f - %.1f), average %.1f us"
              % (k, len(v), statistics.median(v) / 1e3, min(v) / 1e3, max(v) / 1e3, statistics.fmean(v) / 1e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="ns2d_128")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rollout", type=int, default=64)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only-b", type=int, default=0, help="run arm (b) this many times and nothing else (kernel traces)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_eval_stats_time.json"))
    ap.add_argument("--launches", nargs=2, metavar=("KERNEL_TRACE_CSV", "OUT_CSV"),
                    help="host only: per-launch durations of the statistics and the scoring kernel from a kernel trace")
    a = ap.parse_args()
    if a.launches:
        return launches(*a.launches)
    B, T = a.batch, a.rollout
    if not torch.cuda.is_available():
        raise SystemExit("eval_stats_time needs a GPU: a time taken elsewhere says nothing")
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
    eps = float(norm.get("eps", 1e-8))
    eng = model._engine(x)
    eng.set_option("eval_max_steps", max(T, 1024))
    hist = (NBINS, LO, HI)
    every8 = list(range(0, T, 8))
    mean = torch.tensor(norm["mean"], device=dev).reshape(-1, 1, 1) if not isinstance(norm["mean"], float) else norm["mean"]
    std = torch.tensor(norm["std"], device=dev).reshape(-1, 1, 1) if not isinstance(norm["std"], float) else norm["std"]

    def arm_a():
        return eng.rollout_eval(x, y, param=param, **norm)[:2]

    def arm_b():
        return eng.rollout_eval_stats(x, y, param=param, hist=hist, **norm)

    def arm_c():
        return eng.rollout_eval_stats(x, y, param=param, stats_steps=every8, hist=hist, **norm)

    def arm_d():
        out = eng.rollout(x, T, param=param)
        f, s = metrics.relative_l2(out, y, **norm)
        stats = torch.empty((B, T, C, 12), device=dev)
        counts = torch.empty((B, T, C, 2, NBINS + 2), dtype=torch.int64, device=dev)
        for t0 in range(0, T, 16):
            p, q = out[:, t0:t0 + 16] * std + mean, y[:, t0:t0 + 16] * std + mean
            stats[:, t0:t0 + 16] = torch_stats(p, q, eps)
            counts[:, t0:t0 + 16, :, 0] = torch_hist(p, NBINS, LO, HI)
            counts[:, t0:t0 + 16, :, 1] = torch_hist(q, NBINS, LO, HI)
        return f, s, stats, counts

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
    # (d) is torch's reduction order: agreement, not equality -- per column, the largest difference over the column's largest value
    d64 = rd[2].double()
    agree = float(((rb.stats.double() - d64).abs().amax((0, 1, 2)) / d64.abs().amax((0, 1, 2))).max())
    counts_off = int((rb.hist.long() - rd[3]).abs().sum())           # values within rounding of an edge may change bins
    del ra, rb, rd
    times = {k: [] for k in arms}
    for _ in range(a.blocks):
        for k, fn in arms.items():
            times[k].append(block(fn))
    med = {k: statistics.median(v) for k, v in times.items()}
    peaks = {k: peak(fn) for k, fn in arms.items()}
    res = dict(
        tool="eval_stats_time", preset=a.preset, batch=B, rollout=T, blocks=a.blocks, calls_per_block=a.calls, warmup=a.warmup,
        device=torch.cuda.get_device_name(dev), nbins=NBINS, edges=[LO, HI],
        ms_per_call={k: round(v, 3) for k, v in med.items()}, ms_per_call_blocks={k: [round(t, 3) for t in v] for k, v in times.items()},
        a_block_spread=round((max(times["a"]) - min(times["a"])) / med["a"], 4),
        b_over_a=round(med["b"] / med["a"], 4), c_over_a=round(med["c"] / med["a"], 4), d_over_b=round(med["d"] / med["b"], 4),
        peak_bytes_above_resident=peaks, rollout_tensor_bytes=B * T * C * H * W * 4,
        frame_seq_bitwise_equal_a_b=bool(same), b_against_d_worst_relative_difference=agree,
        b_against_d_counts_moved=counts_off, counts_total=2 * B * T * C * H * W)
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

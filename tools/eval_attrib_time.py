"""Validation step with error attribution, three ways, on one box and in one process (default options, arms interleaved):
  (a) Engine.rollout_eval            -- the streaming validation without attribution: the yardstick
  (b) Engine.rollout_eval_attrib     -- every column, no kept frames, no latents
  (d) what exists without the call: Engine.rollout -> [B,T,C,Ly,Lx] in HBM, Engine.rollout(to_x=False) -> the latents, the
      autoencoder over y in chunks -> the reconstruction [B,T,C,Ly,Lx] and the true latents, metrics.relative_l2 three times
      (forecast, reconstruction, latents), and torch for prop and cross, 16 steps at a time
Warm-up, then `blocks` synchronised blocks of `calls` calls per arm; the figure of an arm is the median over its blocks of
(block time / calls), min and max over the blocks beside it; (a)'s spread is (max - min) / median over its blocks.  Peak torch
allocation of each arm above what is resident before it.  The result is merged into a JSON file under the key "T<rollout>".
No speed is promised: (b) pays one encoder and one decoder run per trajectory-step over (a).

    python tools/eval_attrib_time.py [--preset ns2d_128] [--batch 64] [--rollout 64] [--out profiles/rollout_eval_attrib_time.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d out -- python tools/eval_attrib_time.py --only-b 3    # arm (b) alone
    python tools/eval_attrib_time.py --kernel-stats out/<host>/<pid>_kernel_stats.csv profiles/rollout_eval_attrib_trace.json
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

CHUNK = 16
NEW_KERNELS = ("attrib_group_kernel", "latent_err_group_kernel", "attrib_finish_kernel", "metric_group_kernel", "metric_finish_kernel")


def kernel_stats(stats_csv, out_json):
    """rocprofv3's <pid>_kernel_stats.csv -> the rows of the attribution's kernels and the total, as JSON."""
    import csv
    rows, total = {}, 0.0
    with open(stats_csv) as f:
        for row in csv.DictReader(f):
            ns = float(row["TotalDurationNs"])
            total += ns
            for k in NEW_KERNELS:
                if k in row["Name"]:
                    rows[k] = dict(calls=int(row["Calls"]), total_us=round(ns / 1e3, 1), average_us=round(float(row["AverageNs"]) / 1e3, 2),
                                   min_us=round(float(row["MinNs"]) / 1e3, 2), max_us=round(float(row["MaxNs"]) / 1e3, 2))
    doc = dict(tool="eval_attrib_time --kernel-stats", all_kernels_total_us=round(total / 1e3, 1), kernels=rows)
    print(json.dumps(doc))
    with open(out_json, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="ns2d_128")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rollout", type=int, default=64)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only-b", type=int, default=0, help="run arm (b) this many times and nothing else (kernel traces)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_eval_attrib_time.json"))
    ap.add_argument("--kernel-stats", nargs=2, metavar=("KERNEL_STATS_CSV", "OUT_JSON"),
                    help="host only: the attribution kernels' rows of a rocprofv3 --kernel-trace --stats run")
    a = ap.parse_args()
    if a.kernel_stats:
        return kernel_stats(*a.kernel_stats)
    B, T = a.batch, a.rollout
    if not torch.cuda.is_available():
        raise SystemExit("eval_attrib_time needs a GPU: a time taken elsewhere says nothing")
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
    scalar = isinstance(norm["mean"], float) and isinstance(norm["std"], float)
    mean = norm["mean"] if scalar else torch.tensor(norm["mean"], device=dev).reshape(-1, 1, 1)
    std = norm["std"] if scalar else torch.tensor(norm["std"], device=dev).reshape(-1, 1, 1)
    cond = bool(eng.cfg.cond_encoder)

    def arm_a():
        return eng.rollout_eval(x, y, param=param, **norm)[:2]

    def arm_b():
        return eng.rollout_eval_attrib(x, y, param=param, **norm)

    def arm_d():
        out, z = eng.rollout(x, T, param=param, return_latents=True)
        f, s = metrics.relative_l2(out, y, **norm)
        r, zt = torch.empty_like(out), torch.empty_like(z)
        for t in range(T):                                              # the autoencoder over y, one step (B frames) at a time
            zt[:, t] = eng.encode(y[:, t].contiguous(), param) if cond else eng.encode(y[:, t].contiguous())
            r[:, t] = eng.decode(zt[:, t].contiguous())
        rf, rs = metrics.relative_l2(r, y, **norm)
        lf, ls = metrics.relative_l2(z.reshape(B, T, 1, 1, -1), zt.reshape(B, T, 1, 1, -1), eps=eps)
        PP, XX, G = (torch.empty((B, T, C), device=dev) for _ in range(3))
        for t0 in range(0, T, CHUNK):
            sl = slice(t0, t0 + CHUNK)
            if scalar:
                p, q = (out[:, sl] - r[:, sl]) * std, (r[:, sl] - y[:, sl]) * std
            else:
                rr = r[:, sl] * std + mean
                p, q = (out[:, sl] * std + mean) - rr, rr - (y[:, sl] * std + mean)
            g = y[:, sl] * std + mean
            PP[:, sl], XX[:, sl], G[:, sl] = (p * p).sum((-2, -1)), (p * q).sum((-2, -1)), (g * g).sum((-2, -1))
        gc = G.clamp_min(eps)
        gs = G.sum(1).clamp_min(eps)
        return (f, s, rf, rs, (PP / gc).sqrt(), (PP.sum(1) / gs).sqrt(), 2 * XX / gc, 2 * XX.sum(1) / gs, lf.reshape(B, T), ls.reshape(B))

    if a.only_b:
        for _ in range(a.only_b):
            arm_b()
        torch.cuda.synchronize()
        return

    arms = {"a": arm_a, "b": arm_b, "d": arm_d}

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

    def bits(p, q):
        return torch.equal(p.view(torch.int32), q.reshape(p.shape).view(torch.int32))
    same = bits(ra[0], rb.frame) and bits(ra[1], rb.seq)
    stored = [rb.frame, rb.seq, rb.recon_frame, rb.recon_seq, rb.prop_frame, rb.prop_seq, rb.cross_frame, rb.cross_seq,
              rb.latent_frame, rb.latent_seq]
    # the metric columns of (d) are the same kernels on stored tensors (bits); prop and cross of (d) are torch's reductions
    metric_same = all(bits(stored[i], rd[i]) for i in (0, 1, 2, 3, 8, 9))
    agree = max(float((stored[i].double() - rd[i].double()).abs().max() / rd[i].double().abs().max()) for i in (4, 5, 6, 7))
    del ra, rb, rd, stored
    times = {k: [] for k in arms}
    for _ in range(a.blocks):
        for k, fn in arms.items():
            times[k].append(block(fn))
    med = {k: statistics.median(v) for k, v in times.items()}
    peaks = {k: peak(fn) for k, fn in arms.items()}
    res = dict(
        tool="eval_attrib_time", preset=a.preset, batch=B, rollout=T, blocks=a.blocks, calls_per_block=a.calls, warmup=a.warmup,
        device=torch.cuda.get_device_name(dev),
        ms_per_call={k: round(v, 3) for k, v in med.items()}, ms_per_call_min_max={k: [round(min(v), 3), round(max(v), 3)] for k, v in times.items()},
        ms_per_call_blocks={k: [round(t, 3) for t in v] for k, v in times.items()},
        a_block_spread=round((max(times["a"]) - min(times["a"])) / med["a"], 4),
        b_over_a=round(med["b"] / med["a"], 4), d_over_b=round(med["d"] / med["b"], 4),
        peak_bytes_above_resident=peaks, rollout_tensor_bytes=B * T * C * H * W * 4,
        frame_seq_bitwise_equal_a_b=bool(same), metric_columns_bitwise_equal_b_d=bool(metric_same),
        prop_cross_b_against_d_worst_relative_difference=agree)
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

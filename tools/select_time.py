"""What does decoding only the kept steps buy?  One box, one process, NS2d 128x128x3, B = 64, default options:
  (a) full + slice : Engine.rollout(x, T)[:, ::8]           -- the path before keep_steps (all T steps decoded and stored)
  (b) every 4th    : Engine.rollout(x, T, keep_steps=slice(None, None, 4))
  (c) every 8th    : Engine.rollout(x, T, keep_steps=slice(None, None, 8))
  (d) all steps    : Engine.rollout(x, T, keep_steps=range(T))   (the selection path with nothing to skip)
at T = 64 and T = 256.  Warm-up of every arm, then BLOCKS synchronised blocks per arm, interleaved a, b, c, d, a, ...; a block
is ROLLOUTS back-to-back calls between two device synchronisations.  Per arm: median / min / max ms per rollout over the blocks
and the peak torch.cuda.max_memory_allocated of one call; the ratios a/b, a/c, d/a and whether each lies outside the spread of
(a)'s own blocks (a ratio inside [min(a), max(a)] / median(a) says nothing).  Results are compared bit for bit.

    python tools/select_time.py [--out profiles/rollout_select_time.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/select_time.py --trace-arm c --rollout 256
    python tools/select_time.py --trace-dir DIR [--out ...]     # adds the launch count and the chain's kernel-time share
"""
import argparse
import collections
import csv
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ARMS = ("a", "b", "c", "d")
STRIDE = {"b": 4, "c": 8}


def setup(preset, B):
    import torch
    from lns_amd import config, dropin, filler
    dev = torch.device("cuda", 0)
    args = config.preset(preset)
    model = dropin.build_dynamics(args)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(v) for k, v in filler.synthetic_state_dict(shapes, 1).items()})
    model = model.to(dev)
    x = torch.from_numpy(filler.normal("xsel", (B, args.in_channels, args.Ly, args.Lx), 5)).to(dev)
    return args, model._engine(x), x, dev


def arm_fn(eng, x, T, arm):
    if arm == "a":
        return lambda: eng.rollout(x, T)[:, ::8]             # (a view: the slice itself costs nothing and frees nothing)
    if arm == "d":
        return lambda: eng.rollout(x, T, keep_steps=range(T))
    return lambda: eng.rollout(x, T, keep_steps=slice(None, None, STRIDE[arm]))


def measure(a):
    import torch
    args, eng, x, dev = setup(a.preset, a.batch)
    rec = dict(tool="select_time", preset=a.preset, batch=a.batch, blocks=a.blocks, rollouts_per_block=a.rollouts, warmup=a.warmup,
               device=torch.cuda.get_device_name(dev), options="defaults", horizons={})
    for T in a.horizons:
        fns = {k: arm_fn(eng, x, T, k) for k in ARMS}
        for _ in range(a.warmup):
            for k in ARMS:
                fns[k]()
        torch.cuda.synchronize()
        full = eng.rollout(x, T)
        same = {k: bool(torch.equal(fns[k](), full[:, ::STRIDE[k]] if k in STRIDE else full)) for k in ("b", "c", "d")}
        del full
        ms = {k: [] for k in ARMS}
        for _ in range(a.blocks):
            for k in ARMS:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.rollouts):
                    r = fns[k]()
                torch.cuda.synchronize()
                ms[k].append((time.perf_counter() - t0) * 1e3 / a.rollouts)
                del r
        peak = {}
        for k in ARMS:                          # peak allocation of one call above what is resident before it
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            r = fns[k]()
            torch.cuda.synchronize()
            del r
            peak[k] = dict(peak_bytes=torch.cuda.max_memory_allocated(dev), resident_before_bytes=base)
        med = {k: statistics.median(v) for k, v in ms.items()}
        lo, hi = min(ms["a"]) / med["a"], max(ms["a"]) / med["a"]          # (a)'s own block spread, relative
        ratios = {}
        for name, num, den in (("a_over_b", "a", "b"), ("a_over_c", "a", "c"), ("d_over_a", "d", "a")):
            v = med[num] / med[den]
            ratios[name] = dict(value=round(v, 4), outside_spread_of_a=bool(v < lo or v > hi))
        rec["horizons"]["T%d" % T] = dict(
            arms={k: dict(ms_per_rollout=round(med[k], 3), min_ms=round(min(ms[k]), 3), max_ms=round(max(ms[k]), 3),
                          blocks_ms=[round(v, 3) for v in ms[k]], **peak[k]) for k in ARMS},
            spread_of_a_relative=[round(lo, 4), round(hi, 4)], ratios=ratios, kept_steps=dict(b=len(range(0, T, 4)), c=len(range(0, T, 8)), d=T),
            d_slower_than_slowest_a_block=bool(med["d"] > max(ms["a"])), results_bitwise_equal=same)
    return rec


def trace_arm(a):
    """The program of the profiler run: ROLLOUTS calls of one arm and nothing else on the device."""
    import torch
    _, eng, x, _ = setup(a.preset, a.batch)
    T = a.horizons[-1]
    fn = arm_fn(eng, x, T, a.trace_arm)
    for _ in range(a.rollouts):
        fn()
    torch.cuda.synchronize()
    print(json.dumps(dict(trace_arm=a.trace_arm, rollout=T, rollouts=a.rollouts)))


def trace_summary(d, rollouts, T):
    """Launches per rollout and the kernel-time share of the latent chain from a rocprofv3 kernel trace of --trace-arm.
    The overlapped rollout runs the propagator plan, and nothing else, on the engine's side stream: its kernels are the
    queue with the most launches (17+ launches for each of the T steps against one decode launch set per kept step)."""
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    if not rows:
        raise SystemExit("no *kernel_trace.csv under " + d)
    q = collections.defaultdict(list)
    for r in rows:
        q[r["Queue_Id"]].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    busy = {k: sum(e - s for s, e in v) for k, v in q.items()}
    chain = max(q, key=lambda k: len(q[k]))
    total = sum(busy.values())
    span = max(e for v in q.values() for _, e in v) - min(s for v in q.values() for s, _ in v)
    return dict(source="rocprofv3 --kernel-trace --stats, arm (c) on its own, %d rollouts of T = %d, all of them counted" % (rollouts, T),
                launches_total=len(rows), launches_per_rollout=round(len(rows) / rollouts, 1),
                chain_launches_per_rollout=round(len(q[chain]) / rollouts, 1), chain_launches_per_step=round(len(q[chain]) / rollouts / T, 2),
                kernel_ms_per_rollout=round(total / rollouts / 1e6, 3), chain_kernel_ms_per_rollout=round(busy[chain] / rollouts / 1e6, 3),
                chain_share_of_kernel_time=round(busy[chain] / total, 4),
                first_to_last_kernel_ms=round(span / 1e6, 3), chain_busy_over_span=round(busy[chain] / span, 4),
                queues={k: dict(launches=len(v), busy_ms=round(busy[k] / 1e6, 3)) for k, v in q.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="ns2d_128")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--horizons", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--rollout", type=int, default=None, help="one horizon (the trace modes use the last one)")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--rollouts", type=int, default=3, help="rollouts per synchronised block (trace mode: rollouts in all)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_select_time.json"))
    ap.add_argument("--trace-arm", choices=ARMS, default=None)
    ap.add_argument("--trace-dir", default=None)
    a = ap.parse_args()
    if a.rollout:
        a.horizons = [a.rollout]
    if a.trace_arm:
        return trace_arm(a)
    if a.trace_dir:
        rec = json.load(open(a.out))
        rec["trace_arm_c"] = trace_summary(a.trace_dir, a.rollouts, a.horizons[-1])
    else:
        rec = measure(a)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

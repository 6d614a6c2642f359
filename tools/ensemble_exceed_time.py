"""What do the exceedance contingency tables cost?  One box, one process, NS2d 128x128x3, default options, M perturbed members
of each of B trajectories, tools/ensemble_quantile_time.py's protocol and shapes:
  (a) today's path : Engine.rollout_latent(z.view(B * M, ...), T, keep_steps=keep), then metrics.exceedance_table on the stored
                     member fields (elementwise torch ops and bincount on the device)
  (b) the yardstick: Engine.rollout_latent_ensemble(z, T, keep_steps=keep) (mean and variance)
  (c) the new call : Engine.rollout_latent_ensemble_exceed(z, y, T, (thr,), keep_steps=keep), one threshold per channel
at (B, M, T, kept) = (8, 32, 64, 16) and (2, 32, 256, 32).  The truth y is the rollout of each trajectory's first member plus
noise, and the threshold of a channel is the median of its truth, so both outcomes and every forecast value occur.  Warm-up
of all arms, then BLOCKS synchronised blocks per arm, interleaved a, b, c, a, ...; a block is ROLLOUTS back-to-back calls between
two device synchronisations.  Per arm: median / min / max ms per call over the blocks, and the peak
torch.cuda.max_memory_allocated of one call above what is resident before it, measured with the engine's workspace dropped
first (so the workspace is part of the figure; the truth is resident in every arm).  (c)/(b) is set against (b)'s own block
spread (a ratio inside [min(b), max(b)] / median(b) says nothing), and (a)/(c) is reported.

    python tools/ensemble_exceed_time.py [--out profiles/rollout_ensemble_exceed_time.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/ensemble_exceed_time.py --trace-arm c --shape 0
    python tools/ensemble_exceed_time.py --trace-dir DIR --shape 0 [--out ...]     # adds the kernel's time inside the rollout
"""
import argparse
import csv
import ctypes
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ensemble_time import SHAPES, members, setup  # noqa: E402

ARMS = ("a", "b", "c")


def truth(eng, z, T):
    """y [B, T, C, Ly, Lx]: the rollout of each trajectory's first member plus noise of a tenth of its spread, and one
    threshold per channel (the channel's median)"""
    import torch
    y, _ = eng.rollout_latent(z[:, 0].contiguous(), T)
    g = torch.Generator(device=z.device)
    g.manual_seed(11)
    y = (y + 0.1 * y.std() * torch.randn(y.shape, device=z.device, generator=g)).contiguous()
    thr = [float(y[:, ::8, c].median()) for c in range(y.shape[2])]
    return y, thr


def arm_fn(eng, z, y, thr, T, keep, arm):
    from lns_amd import metrics
    B, M = z.shape[:2]
    if arm == "a":
        yk = y[:, keep].contiguous()

        def today():
            full, _ = eng.rollout_latent(z.view((B * M,) + tuple(z.shape[2:])), T, keep_steps=keep)
            return metrics.exceedance_table(full.view((B, M) + tuple(full.shape[1:])), yk, (thr,))
        return today
    if arm == "b":
        return lambda: eng.rollout_latent_ensemble(z, T, keep_steps=keep)
    return lambda: eng.rollout_latent_ensemble_exceed(z, y, T, (thr,), keep_steps=keep)


def measure(a):
    import torch
    from lns_amd import metrics
    args, model, eng, x, dev = setup(a.preset)
    rec = dict(tool="ensemble_exceed_time", preset=a.preset, blocks=a.blocks, rollouts_per_block=a.rollouts, warmup=a.warmup,
               device=torch.cuda.get_device_name(dev), options="defaults", shapes={})
    xper = args.in_channels * args.Ly * args.Lx
    for B, M, T, every in [SHAPES[i] for i in a.shapes]:
        keep = list(range(0, T, every))
        z = members(model, x, B, M)
        y, thr = truth(eng, z, T)
        fns = {k: arm_fn(eng, z, y, thr, T, keep, k) for k in ARMS}
        for _ in range(a.warmup):
            for k in fns:
                fns[k]()
        torch.cuda.synchronize()
        ta, tc = fns["a"](), fns["c"]().table
        torch.cuda.synchronize()
        s = metrics.brier_scores(tc.sum((0, 1), dtype=torch.int64))          # [n_thr = 1, C]: all trajectories and kept steps
        roc = metrics.roc_curve(tc.sum((0, 1), dtype=torch.int64))
        agree = dict(tables_equal=bool(torch.equal(ta, tc)), pixels_per_slice=int(tc[0, 0, 0, 0].sum()), thresholds=thr,
                     base_rate=[round(float(v), 4) for v in s.base_rate[0]], brier=[round(float(v), 5) for v in s.bs[0]],
                     brier_fair=[round(float(v), 5) for v in s.bs_fair[0]], auc=[round(float(v), 4) for v in roc.auc[0]],
                     note="scores of the table summed over trajectories and kept steps, per channel; synthetic weights and a "
                          "synthetic truth: they show that the table is populated, not a forecast quality")
        del ta, tc
        ms = {k: [] for k in fns}
        for _ in range(a.blocks):
            for k in fns:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.rollouts):
                    r = fns[k]()
                torch.cuda.synchronize()
                ms[k].append((time.perf_counter() - t0) * 1e3 / a.rollouts)
                del r
        n_ens = ctypes.c_size_t(0)
        eng._check(eng._L.lns_rollout_ensemble_workspace_bytes(eng._h, B, M, ctypes.byref(n_ens)), "ensemble size")
        peak = {}
        for k in fns:                               # peak of one call above what is resident before it, workspace included
            torch.cuda.synchronize()
            eng._ws.clear()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            r = fns[k]()
            torch.cuda.synchronize()
            del r
            peak[k] = dict(peak_above_resident_bytes=torch.cuda.max_memory_allocated(dev) - base, resident_before_bytes=base)
        out_c = B * len(keep) * args.in_channels * 2 * (M + 1) * 4
        kept_truth = B * len(keep) * xper * 4
        expect_c = n_ens.value + out_c + kept_truth
        memory = dict(ensemble_workspace_bytes=n_ens.value, table_bytes=out_c, kept_truth_copy_bytes=kept_truth, expected_c_bytes=expect_c,
                      c_minus_expected_bytes=peak["c"]["peak_above_resident_bytes"] - expect_c,
                      member_fields_bytes_arm_a=B * M * len(keep) * xper * 4,
                      note="torch's allocator rounds every allocation up to 512 bytes; (c) gathers the kept steps of the truth into "
                           "one contiguous copy; (a) also holds the comparison masks and the int64 counts of exceedance_table")
        med = {k: statistics.median(v) for k, v in ms.items()}
        lo, hi = min(ms["b"]) / med["b"], max(ms["b"]) / med["b"]
        v = med["c"] / med["b"]
        rec["shapes"]["B%d_M%d_T%d_every%d" % (B, M, T, every)] = dict(
            B=B, M=M, T=T, kept_steps=len(keep),
            arms={k: dict(ms_per_call=round(med[k], 3), min_ms=round(min(ms[k]), 3), max_ms=round(max(ms[k]), 3),
                          blocks_ms=[round(t, 3) for t in ms[k]], **peak[k]) for k in fns},
            spread_of_b_relative=[round(lo, 4), round(hi, 4)],
            c_over_b=dict(value=round(v, 4), outside_spread_of_b=bool(v < lo or v > hi)),
            a_over_c=round(med["a"] / med["c"], 4), memory=memory, arms_agree=agree)
        del fns, y, z
    return rec


def trace_arm(a):
    """The program of the profiler run: ROLLOUTS calls of one arm and nothing else on the device (after the truth's rollout)."""
    import torch
    args, model, eng, x, dev = setup(a.preset)
    B, M, T, every = SHAPES[a.shapes[0]]
    z = members(model, x, B, M)
    y, thr = truth(eng, z, T)
    fn = arm_fn(eng, z, y, thr, T, list(range(0, T, every)), a.trace_arm)
    for _ in range(a.rollouts):
        fn()
    torch.cuda.synchronize()
    print(json.dumps(dict(trace_arm=a.trace_arm, shape=SHAPES[a.shapes[0]], rollouts=a.rollouts)))


def trace_summary(d, a):
    """ensemble_exceed_kernel inside the rollout, from a rocprofv3 kernel trace of --trace-arm c."""
    B, M, T, every = SHAPES[a.shapes[0]]
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    if not rows:
        raise SystemExit("no *kernel_trace.csv under " + d)
    dur = {}
    for r in rows:
        dur.setdefault(r["Kernel_Name"].split("(")[0], []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    total = sum(sum(v) for v in dur.values())

    def of(name):
        v = [v for k, v in dur.items() if name in k]
        return v[0] if v else []
    xk = of("ensemble_exceed_kernel")
    per = 3 * 128 * 128
    nbytes = (M + 1) * per * 4 * B
    top = sorted(dur.items(), key=lambda kv: -sum(kv[1]))[:6]
    return dict(source="rocprofv3 --kernel-trace --stats, arm (c) on its own, %d rollouts of shape %s (the trace also holds the one "
                       "rollout that makes the truth)" % (a.rollouts, (B, M, T, every)),
                launches_total=len(rows), kernel_ms_per_rollout=round(total / a.rollouts / 1e6, 3),
                ensemble_exceed_launches=len(xk), ensemble_exceed_median_us=round(statistics.median(xk) / 1e3, 2) if xk else None,
                ensemble_exceed_min_max_us=[round(min(xk) / 1e3, 2), round(max(xk) / 1e3, 2)] if xk else None,
                ensemble_exceed_share_of_kernel_time=round(sum(xk) / total, 5) if xk else None,
                ensemble_exceed_gb_per_s=round(nbytes / statistics.median(xk), 1) if xk else None, algorithmic_bytes_per_launch=nbytes,
                blocks_per_launch=B * 3 * (128 * 128 // 256), global_atomics_per_launch_at_most=B * 3 * (128 * 128 // 256) * 2 * (M + 1),
                top_kernels_share={k[-60:]: round(sum(v) / total, 4) for k, v in top})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="ns2d_128")
    ap.add_argument("--shape", type=int, default=None, help="index into SHAPES (default: both; the trace modes use one)")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--rollouts", type=int, default=3, help="calls per synchronised block (trace mode: calls in all)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_ensemble_exceed_time.json"))
    ap.add_argument("--trace-arm", choices=ARMS, default=None)
    ap.add_argument("--trace-dir", default=None)
    a = ap.parse_args()
    a.shapes = list(range(len(SHAPES))) if a.shape is None else [a.shape]
    if a.trace_arm:
        return trace_arm(a)
    if a.trace_dir:
        rec = json.load(open(a.out))
        rec["trace_arm_c"] = trace_summary(a.trace_dir, a)
    else:
        rec = measure(a)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

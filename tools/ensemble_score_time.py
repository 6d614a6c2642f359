"""What does scoring the ensemble inside the rollout cost, and what does it save?  The method of tools/ensemble_time.py: one
box, one process, NS2d 128x128x3, default options, M perturbed members of each of B trajectories, a random normalised truth:
  (a) without the call : Engine.rollout_latent(z.view(B * M, ...), T, keep_steps=keep), then the scores in torch -- denormalise,
                         mean / var over the members, |v - q|, the pair term in a loop over m, ranks, plane sums, ratios
  (b) no scoring       : Engine.rollout_latent_ensemble(z, T, keep_steps=keep)               (mean and variance)
  (c) the new call     : Engine.rollout_latent_ensemble_eval(z, y, T, keep_steps=keep)       (scores and ranks; no mean, no var)
at (B, M, T, keep) = (8, 32, 64, every 4th step) and (2, 32, 256, every 8th step).  Warm-up of all arms, then BLOCKS synchronised
blocks per arm, interleaved a, b, c, a, ...; a block is ROLLOUTS back-to-back calls between two device synchronisations.  Per
arm: median / min / max ms per call over the blocks, and the peak torch.cuda.max_memory_allocated of one call above what is
resident before it, measured with the engine's workspace dropped first (so the workspace is part of the figure).  (c)'s peak
is compared with what the shapes say: lns_rollout_ensemble_workspace_bytes + scores + seq + rank + the wrapper's contiguous
copy of the kept steps of y.  (c)/(b) is the cost of scoring, set against (b)'s own block spread; (a)/(c) against (a)'s.

    python tools/ensemble_score_time.py [--out profiles/rollout_ensemble_score_time.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/ensemble_score_time.py --trace-arm c --shape 0
    python tools/ensemble_score_time.py --trace-dir DIR --shape 0 [--out ...]     # adds the scoring kernel's time inside the rollout
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from ensemble_time import SHAPES, members, setup  # noqa: E402

NORM = dict(mean=0.37, std=1.9)
EPS = 1e-8


def torch_scores(full, y, M):
    """full [B*M, n, C, H, W] member fields, y [B, n, C, H, W] -> (scores [B, n, C, 4], seq [B, C, 4], rank histogram): what a
    user writes in torch today.  The pair term loops over m so that its temporaries stay [M, ...] and not [M, M, ...]."""
    import torch
    B = y.shape[0]
    HW = y.shape[-2] * y.shape[-1]
    v = (full * NORM["std"] + NORM["mean"]).view((B, M) + tuple(full.shape[1:]))
    q = y * NORM["std"] + NORM["mean"]
    mu, var = v.mean(1), v.var(1)
    a = (v - q[:, None]).abs().sum(1)
    w = torch.zeros_like(q)
    for m in range(M - 1):
        w += (v[:, m:m + 1] - v[:, m + 1:]).abs().sum(1)
    crps = a / M - w / (M * (M - 1))
    rank = (v < q[:, None]).sum(1)
    hist = torch.stack([(rank == k).sum((-2, -1)) for k in range(M + 1)], -1)
    SE, G, V, CR = ((mu - q) ** 2).sum((-2, -1)), (q * q).sum((-2, -1)), var.sum((-2, -1)), crps.sum((-2, -1))
    scores = torch.stack([(SE / G.clamp_min(EPS)).sqrt(), (SE / HW).sqrt(), (V / HW).sqrt(), CR / HW], -1)
    n = y.shape[1]
    seq = torch.stack([(SE.sum(1) / G.sum(1).clamp_min(EPS)).sqrt(), (SE.sum(1) / (n * HW)).sqrt(), (V.sum(1) / (n * HW)).sqrt(),
                       CR.sum(1) / (n * HW)], -1)
    return scores, seq, hist


def arm_fn(eng, z, y, T, keep, arm):
    B, M = z.shape[:2]
    if arm == "a":
        def today():
            full, _ = eng.rollout_latent(z.view((B * M,) + tuple(z.shape[2:])), T, keep_steps=keep)
            return torch_scores(full, y[:, keep], M)
        return today
    if arm == "b":
        return lambda: eng.rollout_latent_ensemble(z, T, keep_steps=keep)
    return lambda: eng.rollout_latent_ensemble_eval(z, y, T, keep_steps=keep, **NORM)


def measure(a):
    import torch
    args, model, eng, x, dev = setup(a.preset)
    rec = dict(tool="ensemble_score_time", preset=a.preset, blocks=a.blocks, rollouts_per_block=a.rollouts, warmup=a.warmup,
               device=torch.cuda.get_device_name(dev), options="defaults", norm=NORM, shapes={})
    C = args.in_channels
    xper = C * args.Ly * args.Lx
    for B, M, T, every in [SHAPES[i] for i in a.shapes]:
        keep = list(range(0, T, every))
        z = members(model, x, B, M)
        g = torch.Generator(device=dev)
        g.manual_seed(11)
        y = torch.randn((B, T, C, args.Ly, args.Lx), device=dev, generator=g)
        fns = {k: arm_fn(eng, z, y, T, keep, k) for k in ("a", "b", "c")}
        for _ in range(a.warmup):
            for k in fns:
                fns[k]()
        torch.cuda.synchronize()
        (sa, qa, ha), s = fns["a"](), fns["c"]()
        torch.cuda.synchronize()
        sc, qc, hc = torch.stack([s.rel_l2, s.rmse, s.spread, s.crps], -1), s.seq, s.rank
        agree = dict(scores_max_rel_diff=[float(((sa[..., i] - sc[..., i]).abs() / sc[..., i].abs().max()).max()) for i in range(4)],
                     seq_max_rel_diff=float(((qa - qc).abs() / qc.abs()).max()), rank_counts_differing=int((ha != hc).sum()),
                     rank_counts=int(hc.numel()),
                     note="torch sums in its own order and fuses x * std + mean: rounding-level differences, and a rank can move at a near-tie")
        del sa, qa, ha, s, sc, qc, hc
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
        nk = len(keep)
        outputs = B * nk * C * 4 * 4 + B * C * 4 * 4 + B * nk * C * (M + 1) * 4
        kept_truth = B * nk * xper * 4
        expect_c = n_ens.value + outputs + kept_truth
        memory = dict(ensemble_workspace_bytes=n_ens.value, scores_seq_rank_bytes=outputs, kept_truth_copy_bytes=kept_truth,
                      member_fields_bytes_arm_a=B * M * nk * xper * 4, expected_c_bytes=expect_c,
                      c_minus_expected_bytes=peak["c"]["peak_above_resident_bytes"] - expect_c,
                      note="(c) = workspace + scores + seq + rank + the wrapper's contiguous y[:, keep]; torch's allocator rounds "
                           "every allocation up to 512 bytes; (a) holds the member fields and torch's temporaries")
        med = {k: statistics.median(v) for k, v in ms.items()}

        def spread(k):
            return [round(min(ms[k]) / med[k], 4), round(max(ms[k]) / med[k], 4)]

        def ratio(num, den, of):
            v = med[num] / med[den]
            lo, hi = spread(of)
            return dict(value=round(v, 4), spread_of=of, outside_spread=bool(v < lo or v > hi))
        rec["shapes"]["B%d_M%d_T%d_every%d" % (B, M, T, every)] = dict(
            B=B, M=M, T=T, kept_steps=nk,
            arms={k: dict(ms_per_call=round(med[k], 3), min_ms=round(min(ms[k]), 3), max_ms=round(max(ms[k]), 3),
                          blocks_ms=[round(t, 3) for t in ms[k]], spread_relative=spread(k), **peak[k]) for k in fns},
            c_over_b=dict(ratio("c", "b", "b"), scoring_ms_per_call=round(med["c"] - med["b"], 3)),
            a_over_c=dict(ratio("a", "c", "a"), c_slower_than_slowest_a_block=bool(med["c"] > max(ms["a"]))),
            memory=memory, arms_agree=agree)
    return rec


def trace_arm(a):
    """The program of the profiler run: ROLLOUTS calls of one arm and nothing else on the device."""
    import torch
    args, model, eng, x, dev = setup(a.preset)
    B, M, T, every = SHAPES[a.shapes[0]]
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    y = torch.randn((B, T, args.in_channels, args.Ly, args.Lx), device=dev, generator=g)
    fn = arm_fn(eng, members(model, x, B, M), y, T, list(range(0, T, every)), a.trace_arm)
    for _ in range(a.rollouts):
        fn()
    torch.cuda.synchronize()
    print(json.dumps(dict(trace_arm=a.trace_arm, shape=SHAPES[a.shapes[0]], rollouts=a.rollouts)))


def trace_summary(d, a):
    """ensemble_score_kernel inside the rollout, and where the kernel time goes, from a rocprofv3 kernel trace of --trace-arm c."""
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

    def one(name):
        v = [t for k, ts in dur.items() if k.endswith(name) for t in ts]
        return dict(launches=len(v), median_us=round(statistics.median(v) / 1e3, 2) if v else None,
                    min_us=round(min(v) / 1e3, 2) if v else None, max_us=round(max(v) / 1e3, 2) if v else None,
                    share_of_kernel_time=round(sum(v) / total, 5) if v else None)
    pixels = B * 3 * 128 * 128
    top = sorted(dur.items(), key=lambda kv: -sum(kv[1]))[:6]
    return dict(source="rocprofv3 --kernel-trace --stats, arm (c) on its own, %d calls of shape %s" % (a.rollouts, (B, M, T, every)),
                launches_total=len(rows), kernel_ms_per_call=round(total / a.rollouts / 1e6, 3),
                ensemble_score_kernel=one("ensemble_score_kernel"), ensemble_score_finish_kernel=one("ensemble_score_finish_kernel"),
                per_launch=dict(blocks=B * 3, pixels=pixels, frame_bytes_read=pixels * (M + 1) * 4,
                                lds_pair_reads=pixels * M * (M - 1) // 2),
                top_kernels_share={k[-60:]: round(sum(v) / total, 4) for k, v in top})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="ns2d_128")
    ap.add_argument("--shape", type=int, default=None, help="index into SHAPES (default: both; the trace modes use one)")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--rollouts", type=int, default=3, help="calls per synchronised block (trace mode: calls in all)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_ensemble_score_time.json"))
    ap.add_argument("--trace-arm", choices=("a", "b", "c"), default=None)
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

"""What do the ensemble quantiles cost?  One box, one process, NS2d 128x128x3, default options, M perturbed members of each of
B trajectories, tools/ensemble_time.py's protocol and shapes:
  (a) today's path : Engine.rollout_latent(z.view(B * M, ...), T, keep_steps=keep), then torch.quantile over the members and a
                     `>` mean for the threshold (torch.quantile takes at most 16 M elements: one call per trajectory and per
                     8 kept steps)
  (b) the yardstick: Engine.rollout_latent_ensemble(z, T, keep_steps=keep) (mean and variance)
  (c) the new call : Engine.rollout_latent_ensemble_quantiles(z, T, (0.05, 0.5, 0.95), (0.5,), keep_steps=keep)
at (B, M, T, kept) = (8, 32, 64, 16) and (2, 32, 256, 32).  Warm-up of all arms, then BLOCKS synchronised blocks per arm,
interleaved a, b, c, a, ...; a block is ROLLOUTS back-to-back calls between two device synchronisations.  Per arm: median /
min / max ms per call over the blocks, and the peak torch.cuda.max_memory_allocated of one call above what is resident before
it, measured with the engine's workspace dropped first (so the workspace is part of the figure); by construction (c)'s peak
is lns_rollout_ensemble_workspace_bytes plus its two outputs.  (c)/(b) is set against (b)'s own block spread (a ratio inside
[min(b), max(b)] / median(b) says nothing), and (a)/(c) is reported.

    python tools/ensemble_quantile_time.py [--out profiles/rollout_ensemble_quantile_time.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/ensemble_quantile_time.py --trace-arm c --shape 0
    python tools/ensemble_quantile_time.py --trace-dir DIR --shape 0 [--out ...]     # adds the kernel's time inside the rollout
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

QUANTILES, THRESHOLD = (0.05, 0.5, 0.95), 0.5
ARMS = ("a", "b", "c")


def arm_fn(eng, z, T, keep, arm):
    import torch
    B, M = z.shape[:2]
    if arm == "a":
        q = torch.tensor(QUANTILES, dtype=torch.float32, device=z.device)

        def today():
            full, _ = eng.rollout_latent(z.view((B * M,) + tuple(z.shape[2:])), T, keep_steps=keep)
            full = full.view((B, M) + tuple(full.shape[1:]))                   # [B, M, n, C, Ly, Lx]
            quant = torch.empty((B, full.shape[2], len(QUANTILES)) + tuple(full.shape[3:]), device=z.device)
            for b in range(B):
                for i in range(0, full.shape[2], 8):
                    quant[b, i:i + 8] = torch.quantile(full[b, :, i:i + 8], q, dim=0).permute(1, 0, 2, 3, 4)
            return quant, (full > THRESHOLD).float().mean(1)
        return today
    if arm == "b":
        return lambda: eng.rollout_latent_ensemble(z, T, keep_steps=keep)
    return lambda: eng.rollout_latent_ensemble_quantiles(z, T, QUANTILES, (THRESHOLD,), keep_steps=keep)


def measure(a):
    import torch
    args, model, eng, x, dev = setup(a.preset)
    rec = dict(tool="ensemble_quantile_time", preset=a.preset, blocks=a.blocks, rollouts_per_block=a.rollouts, warmup=a.warmup,
               device=torch.cuda.get_device_name(dev), options="defaults", quantiles=list(QUANTILES), threshold=THRESHOLD, shapes={})
    xper = args.in_channels * args.Ly * args.Lx
    for B, M, T, every in [SHAPES[i] for i in a.shapes]:
        keep = list(range(0, T, every))
        z = members(model, x, B, M)
        fns = {k: arm_fn(eng, z, T, keep, k) for k in ARMS}
        for _ in range(a.warmup):
            for k in fns:
                fns[k]()
        torch.cuda.synchronize()
        (qa, pa), qc = fns["a"](), fns["c"]()
        torch.cuda.synchronize()
        agree = dict(quantiles_max_abs_diff=float((qa - qc.quantiles).abs().max()), prob_equal=bool(torch.equal(pa[:, :, None], qc.prob)),
                     note="torch.quantile rounds the probabilities to fp32 and interpolates with lerp: rounding-level differences, not bits")
        del qa, pa, qc
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
        out_c = B * len(keep) * (len(QUANTILES) + 1) * xper * 4
        expect_c = n_ens.value + out_c
        memory = dict(ensemble_workspace_bytes=n_ens.value, quantiles_plus_prob_bytes=out_c, expected_c_bytes=expect_c,
                      c_minus_expected_bytes=peak["c"]["peak_above_resident_bytes"] - expect_c,
                      member_fields_bytes_arm_a=B * M * len(keep) * xper * 4,
                      note="torch's allocator rounds every allocation up to 512 bytes; (a) also holds torch.quantile's sorted copy")
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
    return rec


def trace_arm(a):
    """The program of the profiler run: ROLLOUTS calls of one arm and nothing else on the device."""
    import torch
    args, model, eng, x, dev = setup(a.preset)
    B, M, T, every = SHAPES[a.shapes[0]]
    fn = arm_fn(eng, members(model, x, B, M), T, list(range(0, T, every)), a.trace_arm)
    for _ in range(a.rollouts):
        fn()
    torch.cuda.synchronize()
    print(json.dumps(dict(trace_arm=a.trace_arm, shape=SHAPES[a.shapes[0]], rollouts=a.rollouts)))


def trace_summary(d, a):
    """ensemble_quantile_kernel inside the rollout, from a rocprofv3 kernel trace of --trace-arm c."""
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
    qk = [v for k, v in dur.items() if "ensemble_quantile_kernel" in k]
    qk = qk[0] if qk else []
    per = 3 * 128 * 128
    nbytes = (M + len(QUANTILES) + 1) * per * 4 * B
    top = sorted(dur.items(), key=lambda kv: -sum(kv[1]))[:6]
    return dict(source="rocprofv3 --kernel-trace --stats, arm (c) on its own, %d rollouts of shape %s" % (a.rollouts, (B, M, T, every)),
                launches_total=len(rows), kernel_ms_per_rollout=round(total / a.rollouts / 1e6, 3),
                ensemble_quantile_launches=len(qk), ensemble_quantile_median_us=round(statistics.median(qk) / 1e3, 2) if qk else None,
                ensemble_quantile_min_max_us=[round(min(qk) / 1e3, 2), round(max(qk) / 1e3, 2)] if qk else None,
                ensemble_quantile_share_of_kernel_time=round(sum(qk) / total, 5) if qk else None,
                ensemble_quantile_gb_per_s=round(nbytes / statistics.median(qk), 1) if qk else None, algorithmic_bytes_per_launch=nbytes,
                top_kernels_share={k[-60:]: round(sum(v) / total, 4) for k, v in top})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="ns2d_128")
    ap.add_argument("--shape", type=int, default=None, help="index into SHAPES (default: both; the trace modes use one)")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--rollouts", type=int, default=3, help="calls per synchronised block (trace mode: calls in all)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_ensemble_quantile_time.json"))
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

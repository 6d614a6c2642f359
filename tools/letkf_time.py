"""What does the localised ensemble Kalman filter cost?  One box, one process, NS2d 128x128x3, default options, M perturbed members
of each of B trajectories, tools/etkf_time.py's protocol, shapes and observations:
  (a) the yardstick      : Engine.rollout_latent_ensemble(z, T, keep_steps=keep) (mean and variance)
  (b) the global analysis: Engine.rollout_latent_ensemble_analysis(z, y_obs, rinv, T, keep_steps=keep)
  (c) the local analysis : Engine.rollout_latent_ensemble_analysis_local(z, y_obs, rinv, T, 2.0, keep_steps=keep) (radius 2 latent
                           pixels; X_local and wbar_local returned)
at (B, M, T, kept) = (8, 32, 64, 16) and (2, 32, 256, 32).  Warm-up of all arms, then BLOCKS synchronised blocks per arm,
interleaved a, b, c, a, ...; a block is ROLLOUTS back-to-back calls between two device synchronisations.  Per arm: median / min /
max ms per call over the blocks, and the peak torch.cuda.max_memory_allocated of one call above what is resident before it,
measured with the engine's workspace dropped first.  (c)/(a) and (c)/(b) are set against (a)'s own block spread (a ratio inside
[min(a), max(a)] / median(a) says nothing).  Nothing is gated on these numbers.

    python tools/letkf_time.py [--out profiles/rollout_ensemble_analysis_local_time.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/letkf_time.py --trace-arm c --shape 0
    python tools/letkf_time.py --trace-dir DIR --shape 0 [--out ...]     # adds the kernels' launch medians
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
from etkf_time import RHO, RINV, observations  # noqa: E402

ARMS = ("a", "b", "c")
RADIUS = 2.0
KERNELS = ("letkf_patch_gram_kernel", "letkf_combine_kernel", "letkf_update_kernel", "etkf_transform_kernel", "ensemble_transform_kernel")


def arm_fn(eng, z, y, r, T, keep, arm):
    if arm == "a":
        return lambda: eng.rollout_latent_ensemble(z, T, keep_steps=keep)
    if arm == "b":
        return lambda: eng.rollout_latent_ensemble_analysis(z, y, r, T, keep_steps=keep, rho=RHO)
    return lambda: eng.rollout_latent_ensemble_analysis_local(z, y, r, T, RADIUS, keep_steps=keep, rho=RHO)


def measure(a):
    import torch
    args, model, eng, x, dev = setup(a.preset)
    c, h, w = eng.latent_shape()
    rec = dict(tool="letkf_time", preset=a.preset, blocks=a.blocks, rollouts_per_block=a.rollouts, warmup=a.warmup,
               device=torch.cuda.get_device_name(dev), options="defaults", rho=RHO, rinv=RINV, loc_radius=RADIUS, latent=[c, h, w], shapes={},
               not_shown="one box and one run; synthetic weights; the observed fraction (1 / 12 of the values), M = 32 and radius 2 only -- "
                         "M = 64 uses the 4 x 4 register tile and four times the transform's LDS; the radius changes combine alone; a "
                         "dense weight map costs the patch Gram more; no number here is a threshold of a test")
    for B, M, T, every in [SHAPES[i] for i in a.shapes]:
        keep = list(range(0, T, every))
        z = members(model, x, B, M)
        y, r = observations(eng, z, T, keep)
        fns = {k: arm_fn(eng, z, y, r, T, keep, k) for k in ARMS}
        for _ in range(a.warmup):
            for k in fns:
                fns[k]()
        torch.cuda.synchronize()
        rb, rc = fns["b"](), fns["c"]()
        torch.cuda.synchronize()
        dfs_l = (1.0 - (M - 1) / (RHO * rc.lam_local)).sum(-1)
        agree = dict(global_X_of_c_equals_b_rel_l2=float((rc.X - rb.X).norm() / rb.X.norm()), status_local_nonzero=int((rc.status_local != 0).sum()),
                     dfs_global=[round(float(v), 3) for v in (1.0 - (M - 1) / (RHO * rb.lam)).sum(-1)],
                     dfs_local_min_median_max=[round(float(v), 3) for v in (dfs_l.min(), dfs_l.median(), dfs_l.max())],
                     z_rel_l2_c_against_b=float((rc.z - rb.z).norm() / rb.z.norm()),
                     note="the global transform of (c) sums patches where (b) sums slices: equal to rounding, not to the bit")
        del rb, rc
        ms = {k: [] for k in fns}
        for _ in range(a.blocks):
            for k in fns:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.rollouts):
                    res = fns[k]()
                torch.cuda.synchronize()
                ms[k].append((time.perf_counter() - t0) * 1e3 / a.rollouts)
                del res
        n_ens, n_an, n_loc = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
        eng._check(eng._L.lns_rollout_ensemble_workspace_bytes(eng._h, B, M, ctypes.byref(n_ens)), "ensemble size")
        eng._check(eng._L.lns_rollout_ensemble_analysis_workspace_bytes(eng._h, B, M, len(keep), ctypes.byref(n_an)), "analysis size")
        eng._check(eng._L.lns_rollout_ensemble_analysis_local_workspace_bytes(eng._h, B, M, len(keep), ctypes.byref(n_loc)), "local size")
        peak = {}
        for k in fns:                               # peak of one call above what is resident before it, workspace included
            torch.cuda.synchronize()
            eng._ws.clear()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            res = fns[k]()
            torch.cuda.synchronize()
            del res
            peak[k] = dict(peak_above_resident_bytes=torch.cuda.max_memory_allocated(dev) - base, resident_before_bytes=base)
        memory = dict(ensemble_workspace_bytes=n_ens.value, analysis_region_bytes=n_an.value - n_ens.value,
                      local_region_bytes=n_loc.value - n_ens.value, patch_sums_bytes=B * len(keep) * h * w * (M * M + M + 3) * 8,
                      X_local_bytes=B * h * w * M * M * 8)
        med = {k: statistics.median(v) for k, v in ms.items()}
        lo, hi = min(ms["a"]) / med["a"], max(ms["a"]) / med["a"]
        va, vb = med["c"] / med["a"], med["c"] / med["b"]
        rec["shapes"]["B%d_M%d_T%d_every%d" % (B, M, T, every)] = dict(
            B=B, M=M, T=T, kept_steps=len(keep),
            arms={k: dict(ms_per_call=round(med[k], 3), min_ms=round(min(ms[k]), 3), max_ms=round(max(ms[k]), 3),
                          blocks_ms=[round(t, 3) for t in ms[k]], **peak[k]) for k in fns},
            spread_of_a_relative=[round(lo, 4), round(hi, 4)],
            c_over_a=dict(value=round(va, 4), outside_spread_of_a=bool(va < lo or va > hi)),
            c_over_b=dict(value=round(vb, 4), outside_spread_of_a=bool(vb < lo or vb > hi)),
            b_over_a=round(med["b"] / med["a"], 4), memory=memory, arms_agree=agree)
        del fns, y, z
    return rec


def trace_arm(a):
    """The program of the profiler run: ROLLOUTS calls of one arm and nothing else on the device (after the observations' rollout)."""
    import torch
    args, model, eng, x, dev = setup(a.preset)
    B, M, T, every = SHAPES[a.shapes[0]]
    keep = list(range(0, T, every))
    z = members(model, x, B, M)
    y, r = observations(eng, z, T, keep)
    fn = arm_fn(eng, z, y, r, T, keep, a.trace_arm)
    for _ in range(a.rollouts):
        fn()
    torch.cuda.synchronize()
    print(json.dumps(dict(trace_arm=a.trace_arm, shape=SHAPES[a.shapes[0]], rollouts=a.rollouts)))


def trace_summary(d, a):
    """the filter's kernels inside the rollout, from a rocprofv3 kernel trace of --trace-arm c; the transform kernel's launches are
    split by grid size into the B * h * w-block launch (per domain) and the B-block one (global)"""
    B, M, T, every = SHAPES[a.shapes[0]]
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    if not rows:
        raise SystemExit("no *kernel_trace.csv under " + d)
    dur, grids = {}, {}
    for r in rows:
        name = r["Kernel_Name"].split("(")[0]
        t = int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        dur.setdefault(name, []).append(t)
        if "etkf_transform_kernel" in name:
            grids.setdefault(int(r.get("Grid_Size_X", r.get("Grid_Size", 0)) or 0), []).append(t)
    total = sum(sum(v) for v in dur.values())
    out = dict(source="rocprofv3 --kernel-trace --stats, arm (c) on its own, %d calls of shape %s (the trace also holds the one rollout "
                      "that makes the observations)" % (a.rollouts, (B, M, T, every)),
               launches_total=len(rows), kernel_ms_per_call=round(total / a.rollouts / 1e6, 3), kernels={})
    for name in KERNELS:
        v = [t for k, ts in dur.items() if name in k for t in ts]
        out["kernels"][name] = dict(launches=len(v), median_us=round(statistics.median(v) / 1e3, 2) if v else None,
                                    min_max_us=[round(min(v) / 1e3, 2), round(max(v) / 1e3, 2)] if v else None,
                                    share_of_kernel_time=round(sum(v) / total, 5) if v else None)
    out["etkf_transform_kernel_by_grid_size_x"] = {str(g): dict(launches=len(v), median_us=round(statistics.median(v) / 1e3, 2))
                                                   for g, v in sorted(grids.items())}
    top = sorted(dur.items(), key=lambda kv: -sum(kv[1]))[:6]
    out["top_kernels_share"] = {k[-60:]: round(sum(v) / total, 4) for k, v in top}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="ns2d_128")
    ap.add_argument("--shape", type=int, default=None, help="index into SHAPES (default: both; the trace modes use one)")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--rollouts", type=int, default=3, help="calls per synchronised block (trace mode: calls in all)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_ensemble_analysis_local_time.json"))
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

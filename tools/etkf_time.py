"""What does the ensemble transform Kalman filter cost?  One box, one process, NS2d 128x128x3, default options, M perturbed
members of each of B trajectories, tools/ensemble_time.py's protocol and shapes:
  (a) the yardstick    : Engine.rollout_latent_ensemble(z, T, keep_steps=keep) (mean and variance)
  (b) the new call     : Engine.rollout_latent_ensemble_analysis(z, y_obs, rinv, T, keep_steps=keep) (no mean, no variance)
  (c) what exists without it: Engine.rollout_latent(z.view(B * M, ...), T, keep_steps=keep), then the Gram by a float64 einsum
                         on the stored member fields, torch.linalg.eigh and the update in torch
at (B, M, T, kept) = (8, 32, 64, 16) and (2, 32, 256, 32).  Every 4th pixel of channel 0 is observed at every kept step
(rinv = 1e2 there); the observations are the rollout of each trajectory's first member plus noise.  Warm-up of all arms, then
BLOCKS synchronised blocks per arm, interleaved a, b, c, a, ...; a block is ROLLOUTS back-to-back calls between two device
synchronisations.  Per arm: median / min / max ms per call over the blocks, and the peak torch.cuda.max_memory_allocated of one
call above what is resident before it, measured with the engine's workspace dropped first (so the workspace is part of the
figure; the observations are resident in every arm).  (b)/(a) is set against (a)'s own block spread (a ratio inside
[min(a), max(a)] / median(a) says nothing), and (c)/(b) is reported.  Nothing is gated on these numbers.

    python tools/etkf_time.py [--out profiles/rollout_ensemble_analysis_time.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/etkf_time.py --trace-arm b --shape 0
    python tools/etkf_time.py --trace-dir DIR --shape 0 [--out ...]     # adds the three kernels' launch medians
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
RHO, RINV = 1.0, 1.0e2
KERNELS = ("ensemble_obs_gram_kernel", "ensemble_obs_gram_finish_kernel", "etkf_transform_kernel", "ensemble_transform_kernel")


def observations(eng, z, T, keep):
    """y_obs [B, n_keep, C, Ly, Lx]: the rollout of each trajectory's first member plus noise of a tenth of its spread; rinv
    [C, Ly, Lx]: every 4th pixel of channel 0"""
    import torch
    y, _ = eng.rollout_latent(z[:, 0].contiguous(), T, keep_steps=keep)
    g = torch.Generator(device=z.device)
    g.manual_seed(11)
    y = (y + 0.1 * y.std() * torch.randn(y.shape, device=z.device, generator=g)).contiguous()
    r = torch.zeros(tuple(y.shape[2:]), device=z.device)
    r[0].view(-1)[::4] = RINV
    return y, r


def torch_filter(full, z_last, y, r, B, M):
    """arm (c)'s filter on stored member fields [B * M, n, C, H, W]: float64 einsum, torch.linalg.eigh, the update"""
    import torch
    n = full.shape[1]
    f = full.view(B, M, n, -1).double()
    ybar = f.mean(1, keepdim=True)
    Y = f - ybar
    d = y.view(B, n, -1).double() - ybar[:, 0]
    Yw = Y * r.view(1, 1, 1, -1).double()
    S = torch.einsum("bmnp,bknp->bmk", Yw, Y)
    g = torch.einsum("bmnp,bnp->bm", Yw, d)
    A = S + (M - 1) / RHO * torch.eye(M, dtype=torch.float64, device=full.device)
    lam, Q = torch.linalg.eigh(A)
    wbar = torch.einsum("bik,bk->bi", Q, torch.einsum("bik,bi->bk", Q, g) / lam)
    W = torch.einsum("bik,bjk->bij", Q * torch.sqrt((M - 1) / lam)[:, None], Q)
    X = W + wbar[:, :, None]
    zf = z_last.view(B, M, -1).double()
    zbar = zf.mean(1, keepdim=True)
    return (zbar + torch.einsum("bkn,bkm->bmn", zf - zbar, X)).float(), X


def arm_fn(eng, z, y, r, T, keep, arm):
    B, M = z.shape[:2]
    if arm == "a":
        return lambda: eng.rollout_latent_ensemble(z, T, keep_steps=keep)
    if arm == "b":
        return lambda: eng.rollout_latent_ensemble_analysis(z, y, r, T, keep_steps=keep, rho=RHO)

    def existing():
        full, zl = eng.rollout_latent(z.view((B * M,) + tuple(z.shape[2:])), T, keep_steps=keep)
        return torch_filter(full, zl, y, r, B, M)
    return existing


def measure(a):
    import torch
    args, model, eng, x, dev = setup(a.preset)
    rec = dict(tool="etkf_time", preset=a.preset, blocks=a.blocks, rollouts_per_block=a.rollouts, warmup=a.warmup,
               device=torch.cuda.get_device_name(dev), options="defaults", rho=RHO, rinv=RINV, shapes={},
               not_shown="one box and one run; synthetic weights; the observed fraction (1 / 12 of the values) and M = 32 only -- the "
                         "Gram kernel reads every rinv but loads members at observed values only, so a dense map costs more; M = 64 "
                         "uses the 4 x 4 register tile, M <= 32 the 2 x 2 one; arm (c) is one plain way to write the filter in torch, "
                         "not a tuned one; no number here is a threshold of a test")
    xper = args.in_channels * args.Ly * args.Lx
    for B, M, T, every in [SHAPES[i] for i in a.shapes]:
        keep = list(range(0, T, every))
        z = members(model, x, B, M)
        y, r = observations(eng, z, T, keep)
        fns = {k: arm_fn(eng, z, y, r, T, keep, k) for k in ARMS}
        for _ in range(a.warmup):
            for k in fns:
                fns[k]()
        torch.cuda.synchronize()
        rb, (zc, Xc) = fns["b"](), fns["c"]()
        torch.cuda.synchronize()
        agree = dict(X_rel_l2_b_against_c=float((rb.X - Xc).norm() / Xc.norm()), z_rel_l2_b_against_c=float((rb.z.view(zc.shape) - zc).norm() / zc.norm()),
                     status=rb.status.tolist(), dfs=[round(float(v), 3) for v in (1.0 - (M - 1) / (RHO * rb.lam)).sum(-1)],
                     observed_values_per_step=int(rb.stat[0, 0, 2]),
                     note="(c) sums in another order and takes eigh's eigenvectors: the two agree to rounding, not to the bit")
        del rb, zc, Xc
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
        n_ens, n_an = ctypes.c_size_t(0), ctypes.c_size_t(0)
        eng._check(eng._L.lns_rollout_ensemble_workspace_bytes(eng._h, B, M, ctypes.byref(n_ens)), "ensemble size")
        eng._check(eng._L.lns_rollout_ensemble_analysis_workspace_bytes(eng._h, B, M, len(keep), ctypes.byref(n_an)), "analysis size")
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
        memory = dict(ensemble_workspace_bytes=n_ens.value, analysis_workspace_bytes=n_an.value,
                      analysis_region_bytes=n_an.value - n_ens.value, member_fields_bytes_arm_c=B * M * len(keep) * xper * 4,
                      note="(b): the workspace, z_analysis, X, wbar, lam, stat, status; (c) also holds the member fields in fp32 and "
                           "their anomalies in float64")
        med = {k: statistics.median(v) for k, v in ms.items()}
        lo, hi = min(ms["a"]) / med["a"], max(ms["a"]) / med["a"]
        v = med["b"] / med["a"]
        rec["shapes"]["B%d_M%d_T%d_every%d" % (B, M, T, every)] = dict(
            B=B, M=M, T=T, kept_steps=len(keep),
            arms={k: dict(ms_per_call=round(med[k], 3), min_ms=round(min(ms[k]), 3), max_ms=round(max(ms[k]), 3),
                          blocks_ms=[round(t, 3) for t in ms[k]], **peak[k]) for k in fns},
            spread_of_a_relative=[round(lo, 4), round(hi, 4)],
            b_over_a=dict(value=round(v, 4), outside_spread_of_a=bool(v < lo or v > hi)),
            c_over_b=round(med["c"] / med["b"], 4), memory=memory, arms_agree=agree)
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
    """the filter's kernels inside the rollout, from a rocprofv3 kernel trace of --trace-arm b"""
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
    out = dict(source="rocprofv3 --kernel-trace --stats, arm (b) on its own, %d calls of shape %s (the trace also holds the one rollout "
                      "that makes the observations)" % (a.rollouts, (B, M, T, every)),
               launches_total=len(rows), kernel_ms_per_call=round(total / a.rollouts / 1e6, 3), kernels={})
    for name in KERNELS:
        v = [t for k, ts in dur.items() if name in k and (name != "ensemble_obs_gram_kernel" or "finish" not in k) for t in ts]
        out["kernels"][name] = dict(launches=len(v), median_us=round(statistics.median(v) / 1e3, 2) if v else None,
                                    min_max_us=[round(min(v) / 1e3, 2), round(max(v) / 1e3, 2)] if v else None,
                                    share_of_kernel_time=round(sum(v) / total, 5) if v else None)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_ensemble_analysis_time.json"))
    ap.add_argument("--trace-arm", choices=ARMS, default=None)
    ap.add_argument("--trace-dir", default=None)
    a = ap.parse_args()
    a.shapes = list(range(len(SHAPES))) if a.shape is None else [a.shape]
    if a.trace_arm:
        return trace_arm(a)
    if a.trace_dir:
        rec = json.load(open(a.out))
        rec["trace_arm_b"] = trace_summary(a.trace_dir, a)
    else:
        rec = measure(a)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

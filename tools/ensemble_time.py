"""What does the ensemble rollout buy?  One box, one process, NS2d 128x128x3, default options, M perturbed members of each
of B trajectories:
  (a) today's path : Engine.rollout_latent(z.view(B * M, ...), T, keep_steps=keep), then mean(1) and var(1) in torch
  (b) the new call : Engine.rollout_latent_ensemble(z, T, keep_steps=keep)
at (B, M, T, keep) = (8, 32, 64, every 4th step) and (2, 32, 256, every 8th step).  Warm-up of both arms, then BLOCKS
synchronised blocks per arm, interleaved a, b, a, ...; a block is ROLLOUTS back-to-back calls between two device
synchronisations.  Per arm: median / min / max ms per call over the blocks, and the peak torch.cuda.max_memory_allocated of
one call above what is resident before it, measured with the engine's workspace dropped first (so the workspace is part of
the figure) and compared with what the shapes say: (b) = lns_rollout_ensemble_workspace_bytes + mean + var, where the
workspace is lns_prepare(B * M) plus the growth documented in include/lns.h.  (a)/(b) is set against (a)'s own block spread
(a ratio inside [min(a), max(a)] / median(a) says nothing).  The reduction kernel on its own (lns_op_ensemble_stats on one
frame buffer [B, M, C * Ly * Lx], HIP events around REPS launches) gives its bytes per second on the algorithmic bytes
(2 M + 2) * per * 4 per trajectory: it reads the members twice.

    python tools/ensemble_time.py [--out profiles/rollout_ensemble_time.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/ensemble_time.py --trace-arm b --shape 0
    python tools/ensemble_time.py --trace-dir DIR --shape 0 [--out ...]     # adds the kernel's time inside the rollout
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

SHAPES = ((8, 32, 64, 4), (2, 32, 256, 8))          # (B, M, T, keep every k-th step)
NOISE = 0.05
REPS = 20


def setup(preset):
    import torch
    from lns_amd import config, dropin, filler
    dev = torch.device("cuda", 0)
    args = config.preset(preset)
    model = dropin.build_dynamics(args)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(v) for k, v in filler.synthetic_state_dict(shapes, 1).items()})
    model = model.to(dev)
    x = torch.from_numpy(filler.normal("xens", (max(s[0] for s in SHAPES), args.in_channels, args.Ly, args.Lx), 5)).to(dev)
    return args, model, model._engine(x), x, dev


def members(model, x, B, M):
    import torch
    g = torch.Generator(device=x.device)
    g.manual_seed(7)
    z0 = model.x_to_z(x[:B].contiguous())
    z = z0[:, None] + torch.randn((B, M) + tuple(z0.shape[1:]), device=x.device, generator=g) * NOISE
    z[:, 0] = z0
    return z.contiguous()


def arm_fn(eng, z, T, keep, arm):
    B, M = z.shape[:2]
    if arm == "a":
        def today():
            full, _ = eng.rollout_latent(z.view((B * M,) + tuple(z.shape[2:])), T, keep_steps=keep)
            full = full.view((B, M) + tuple(full.shape[1:]))
            return full.mean(1), full.var(1)
        return today
    return lambda: eng.rollout_latent_ensemble(z, T, keep_steps=keep)


def up(v):
    return (v + 255) // 256 * 256


def kernel_alone(eng, args, B, M, dev):
    """ensemble_stats_kernel on one frame buffer of the rollout's shape, REPS launches between two HIP events."""
    import torch
    from lns_amd import _lib
    L = _lib.lib()
    per = args.in_channels * args.Ly * args.Lx
    frames = torch.randn((B, M, per), device=dev)
    mean, var = torch.empty((B, per), device=dev), torch.empty((B, per), device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for _ in range(3):
        assert L.lns_op_ensemble_stats(frames.data_ptr(), B, M, per, mean.data_ptr(), var.data_ptr(), stream) == 0
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        L.lns_op_ensemble_stats(frames.data_ptr(), B, M, per, mean.data_ptr(), var.data_ptr(), stream)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / REPS
    nbytes = (2 * M + 2) * per * 4 * B
    return dict(frame_buffer_bytes=B * M * per * 4, algorithmic_bytes=nbytes, us_per_launch=round(us, 2),
                gb_per_s=round(nbytes / us / 1e3, 1),
                note="events around %d back-to-back op calls, each of which synchronises the stream: launch gaps included" % REPS)


def measure(a):
    import torch
    args, model, eng, x, dev = setup(a.preset)
    rec = dict(tool="ensemble_time", preset=a.preset, blocks=a.blocks, rollouts_per_block=a.rollouts, warmup=a.warmup,
               device=torch.cuda.get_device_name(dev), options="defaults", noise_level=NOISE, shapes={})
    c, h, w = eng.latent_shape()
    xper = args.in_channels * args.Ly * args.Lx
    for B, M, T, every in [SHAPES[i] for i in a.shapes]:
        N = B * M
        keep = list(range(0, T, every))
        z = members(model, x, B, M)
        fns = {k: arm_fn(eng, z, T, keep, k) for k in ("a", "b")}
        for _ in range(a.warmup):
            for k in fns:
                fns[k]()
        torch.cuda.synchronize()
        (ma, va), (mb, vb) = fns["a"](), fns["b"]()
        torch.cuda.synchronize()
        agree = dict(mean_max_abs_diff=float((ma - mb).abs().max()), var_max_rel_diff=float(((va - vb).abs() / vb.abs().max()).max()),
                     note="torch's mean / var sum in torch's order: rounding-level differences, not bits")
        del ma, va, mb, vb
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
        n_prep, n_sel, n_ens = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
        eng._check(eng._L.lns_prepare(eng._h, N, ctypes.byref(n_prep)), "lns_prepare")
        eng._check(eng._L.lns_rollout_select_workspace_bytes(eng._h, N, ctypes.byref(n_sel)), "select size")
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
        out_bytes = B * len(keep) * xper * 4
        growth = up(n_prep.value) - n_prep.value + 2 * up(N * c * h * w * 4) + 3 * up(1 * N * xper * 4)   # defaults: 3 streams, 1 step
        expect_b = n_prep.value + growth + 2 * out_bytes
        members_bytes = N * len(keep) * xper * 4
        expect_a = n_sel.value + members_bytes + 2 * out_bytes
        memory = dict(lns_prepare_bytes=n_prep.value, select_workspace_bytes=n_sel.value, ensemble_workspace_bytes=n_ens.value,
                      workspace_growth_from_shapes=growth, growth_matches_size_query=bool(n_prep.value + growth == n_ens.value),
                      mean_plus_var_bytes=2 * out_bytes, member_fields_bytes_arm_a=members_bytes,
                      expected_b_bytes=expect_b, b_minus_expected_bytes=peak["b"]["peak_above_resident_bytes"] - expect_b,
                      expected_a_at_least_bytes=expect_a, a_minus_expected_bytes=peak["a"]["peak_above_resident_bytes"] - expect_a,
                      note="torch's allocator rounds every allocation up to 512 bytes; (a) also holds torch's reduction temporaries")
        med = {k: statistics.median(v) for k, v in ms.items()}
        lo, hi = min(ms["a"]) / med["a"], max(ms["a"]) / med["a"]
        v = med["a"] / med["b"]
        rec["shapes"]["B%d_M%d_T%d_every%d" % (B, M, T, every)] = dict(
            B=B, M=M, T=T, kept_steps=len(keep),
            arms={k: dict(ms_per_call=round(med[k], 3), min_ms=round(min(ms[k]), 3), max_ms=round(max(ms[k]), 3),
                          blocks_ms=[round(t, 3) for t in ms[k]], **peak[k]) for k in fns},
            spread_of_a_relative=[round(lo, 4), round(hi, 4)],
            a_over_b=dict(value=round(v, 4), outside_spread_of_a=bool(v < lo or v > hi), b_slower_than_slowest_a_block=bool(med["b"] > max(ms["a"]))),
            memory=memory, arms_agree=agree, ensemble_stats_kernel_alone=kernel_alone(eng, args, B, M, dev))
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
    """ensemble_stats_kernel inside the rollout, and where the kernel time goes, from a rocprofv3 kernel trace of --trace-arm b."""
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
    ens = [v for k, v in dur.items() if "ensemble_stats_kernel" in k]
    ens = ens[0] if ens else []
    per = 3 * 128 * 128
    nbytes = (2 * M + 2) * per * 4 * B
    top = sorted(dur.items(), key=lambda kv: -sum(kv[1]))[:6]
    return dict(source="rocprofv3 --kernel-trace --stats, arm (b) on its own, %d rollouts of shape %s" % (a.rollouts, (B, M, T, every)),
                launches_total=len(rows), kernel_ms_per_rollout=round(total / a.rollouts / 1e6, 3),
                ensemble_stats_launches=len(ens), ensemble_stats_median_us=round(statistics.median(ens) / 1e3, 2) if ens else None,
                ensemble_stats_share_of_kernel_time=round(sum(ens) / total, 5) if ens else None,
                ensemble_stats_gb_per_s=round(nbytes / statistics.median(ens), 1) if ens else None, algorithmic_bytes_per_launch=nbytes,
                top_kernels_share={k[-60:]: round(sum(v) / total, 4) for k, v in top})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="ns2d_128")
    ap.add_argument("--shape", type=int, default=None, help="index into SHAPES (default: both; the trace modes use one)")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--rollouts", type=int, default=3, help="calls per synchronised block (trace mode: calls in all)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_ensemble_time.json"))
    ap.add_argument("--trace-arm", choices=("a", "b"), default=None)
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

"""Validation step with flow diagnostics, four ways, on one box and in one process (default options, arms interleaved):
  (a) Engine.rollout_eval                          -- the streaming validation without diagnostics: the yardstick
  (b) Engine.rollout_eval_flow, diagnostics and a 64-bin vorticity histogram of every step
  (c) Engine.rollout_eval_flow, of every 8th step
  (d) what exists without the call: Engine.rollout -> [B,T,C,Ly,Lx] in HBM -> metrics.relative_l2 -> the same twelve
      quantities and the histograms in torch on the stored tensor, 16 steps at a time
Warm-up, then `blocks` synchronised blocks of `calls` calls per arm; the figure of an arm is the median over its blocks of
(block time / calls), (a)'s spread is (max - min) / median over its blocks.  Peak torch allocation of each arm above what
is resident before it.  The result is merged into a JSON file under the key "T<rollout>".

    python tools/eval_flow_time.py [--preset ns2d_128] [--batch 64] [--rollout 64] [--out profiles/rollout_eval_flow_time.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d out -- python tools/eval_flow_time.py --only-b 3    # arm (b) alone
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
from eval_stats_time import torch_hist  # noqa: E402

NBINS, LO, HI = 64, -8.0, 8.0
U, V, DX, DY = 0, 1, 1.0, 1.0


def torch_deriv(f, dim, wall, d):
    """Central differences of f [..., H, W] along dim: wrapped, or one-sided at the two ends (numpy.gradient, edge_order=1)."""
    if not wall:
        return (torch.roll(f, -1, dim) - torch.roll(f, 1, dim)) / (2.0 * d)
    return torch.gradient(f, spacing=d, dim=dim, edge_order=1)[0]


def torch_flow(p, q, bc, eps):
    """p, q [B, t, C, H, W] denormalised -> ([B, t, 12] (metrics.FLOW_STATS), vorticity of p, of q) with torch's reductions."""
    def fields(x):
        u, v = x[:, :, U], x[:, :, V]
        w = torch_deriv(v, -1, bc[1], DX) - torch_deriv(u, -2, bc[0], DY)
        dv = torch_deriv(u, -1, bc[1], DX) + torch_deriv(v, -2, bc[0], DY)
        return u, v, w, dv
    (up, vp, wp, dp), (uq, vq, wq, dq) = fields(p), fields(q)
    d = (-2, -1)
    n = p.shape[-2] * p.shape[-1]
    kp, kq = (up * up + vp * vp).sum(d), (uq * uq + vq * vq).sum(d)
    wpp, wqq = (wp * wp).sum(d), (wq * wq).sum(d)
    cols = [0.5 * kp / n, 0.5 * kq / n, 0.5 * wpp / n, 0.5 * wqq / n, ((dp * dp).sum(d) / n).sqrt(), ((dq * dq).sum(d) / n).sqrt(),
            (((wp - wq) ** 2).sum(d) / wqq.clamp_min(eps)).sqrt(), (wp * wq).sum(d) / ((wpp.sqrt() + eps) * (wqq.sqrt() + eps)),
            (((up - uq) ** 2 + (vp - vq) ** 2).sum(d) / kq.clamp_min(eps)).sqrt(), wp.abs().amax(d), wq.abs().amax(d), dp.abs().amax(d)]
    return torch.stack(cols, -1), wp, wq


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="ns2d_128")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rollout", type=int, default=64)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only-b", type=int, default=0, help="run arm (b) this many times and nothing else (kernel traces)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_eval_flow_time.json"))
    a = ap.parse_args()
    B, T = a.batch, a.rollout
    if not torch.cuda.is_available():
        raise SystemExit("eval_flow_time needs a GPU: a time taken elsewhere says nothing")
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
    bc = metrics.flow_boundary("auto", eng.cfg)
    vhist = (NBINS, LO, HI)
    flow_kw = dict(u=U, v=V, dx=DX, dy=DY, boundary="auto", vort_hist=vhist)
    every8 = list(range(0, T, 8))
    mean = torch.tensor(norm["mean"], device=dev).reshape(-1, 1, 1) if not isinstance(norm["mean"], float) else norm["mean"]
    std = torch.tensor(norm["std"], device=dev).reshape(-1, 1, 1) if not isinstance(norm["std"], float) else norm["std"]

    def arm_a():
        return eng.rollout_eval(x, y, param=param, **norm)[:2]

    def arm_b():
        return eng.rollout_eval_flow(x, y, param=param, **flow_kw, **norm)

    def arm_c():
        return eng.rollout_eval_flow(x, y, param=param, flow_steps=every8, **flow_kw, **norm)

    def arm_d():
        out = eng.rollout(x, T, param=param)
        f, s = metrics.relative_l2(out, y, **norm)
        flow = torch.empty((B, T, 12), device=dev)
        counts = torch.empty((B, T, 2, NBINS + 2), dtype=torch.int64, device=dev)
        for t0 in range(0, T, 16):
            p, q = out[:, t0:t0 + 16] * std + mean, y[:, t0:t0 + 16] * std + mean
            flow[:, t0:t0 + 16], wp, wq = torch_flow(p, q, bc, eps)
            counts[:, t0:t0 + 16, 0] = torch_hist(wp[:, :, None], NBINS, LO, HI)[:, :, 0]
            counts[:, t0:t0 + 16, 1] = torch_hist(wq[:, :, None], NBINS, LO, HI)[:, :, 0]
        return f, s, flow, counts

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
    agree = float(((rb.flow.double() - d64).abs().amax((0, 1)) / d64.abs().amax((0, 1))).max())
    counts_off = int((rb.hist.long() - rd[3]).abs().sum())           # values within rounding of an edge may change bins
    del ra, rb, rd
    times = {k: [] for k in arms}
    for _ in range(a.blocks):
        for k, fn in arms.items():
            times[k].append(block(fn))
    med = {k: statistics.median(v) for k, v in times.items()}
    peaks = {k: peak(fn) for k, fn in arms.items()}
    spread = (max(times["a"]) - min(times["a"])) / med["a"]
    ratios = dict(b_over_a=med["b"] / med["a"], c_over_a=med["c"] / med["a"], d_over_b=med["d"] / med["b"])
    res = dict(
        tool="eval_flow_time", preset=a.preset, batch=B, rollout=T, blocks=a.blocks, calls_per_block=a.calls, warmup=a.warmup,
        device=torch.cuda.get_device_name(dev), nbins=NBINS, edges=[LO, HI], boundary=list(bc), channels=[U, V], spacing=[DX, DY],
        ms_per_call={k: round(v, 3) for k, v in med.items()}, ms_per_call_blocks={k: [round(t, 3) for t in v] for k, v in times.items()},
        a_block_spread=round(spread, 4), **{k: round(v, 4) for k, v in ratios.items()},
        inside_a_block_spread={k: bool(abs(v - 1.0) <= spread) for k, v in ratios.items()},
        peak_bytes_above_resident=peaks, rollout_tensor_bytes=B * T * C * H * W * 4,
        frame_seq_bitwise_equal_a_b=bool(same), b_against_d_worst_relative_difference=agree,
        b_against_d_counts_moved=counts_off, counts_total=2 * B * T * H * W)
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

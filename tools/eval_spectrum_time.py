"""Validation step with energy spectra, four ways, on one box and in one process (default options, arms interleaved):
  (a) Engine.rollout_eval                          -- the streaming validation without spectra: the yardstick
  (b) Engine.rollout_eval_spectrum, every step
  (c) Engine.rollout_eval_spectrum, every 8th step
  (d) what exists without the call: Engine.rollout -> [B,T,C,Ly,Lx] in HBM -> metrics.relative_l2 -> spectra of forecast,
      truth and error from torch.fft.rfft2 with a shell index_add (left out, and said so, where torch.fft is not usable)
Warm-up, then `blocks` synchronised blocks of `calls` calls per arm; the figure of an arm is the median over its blocks of
(block time / calls), (a)'s spread is (max - min) / median over its blocks.  Peak torch allocation of each arm above what
is resident before it.  The result is merged into a JSON file under the key "T<rollout>".

    python tools/eval_spectrum_time.py [--preset ns2d_128] [--batch 64] [--rollout 64] [--out profiles/rollout_eval_spectrum_time.json]
    rocprofv3 --kernel-trace --stats -d out -- python tools/eval_spectrum_time.py --only-b 3      # arm (b) alone, for a kernel trace
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


def shell_index(H, W, device):
    """[H * Wh] int64 shell of every stored mode and [Wh] conjugate weights (the integer rule of include/lns.h)."""
    Wh = W // 2 + 1
    ky = torch.arange(H, device=device)
    ky = torch.where(ky <= H // 2, ky, ky - H)
    kx = torch.arange(Wh, device=device)
    r2 = ky[:, None] ** 2 + kx[None, :] ** 2
    s = torch.round(torch.sqrt(r2.double())).long()
    s = torch.where(s * (s - 1) >= r2, s - 1, s)
    s = torch.where(s * (s + 1) < r2, s + 1, s)
    s = torch.where(r2 == 0, torch.zeros_like(s), s)
    w = torch.full((Wh,), 2.0, device=device)
    w[0] = 1.0
    if W % 2 == 0:
        w[W // 2] = 1.0
    return s.reshape(-1), w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="ns2d_128")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rollout", type=int, default=64)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only-b", type=int, default=0, help="run arm (b) this many times and nothing else (kernel traces)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_eval_spectrum_time.json"))
    a = ap.parse_args()
    B, T = a.batch, a.rollout
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
    eng = model._engine(x)
    eng.set_option("eval_max_steps", max(T, 1024))
    S = metrics.spectrum_bins(H, W)
    every8 = list(range(0, T, 8))
    idx, wgt = shell_index(H, W, dev)
    mean = torch.tensor(norm["mean"], device=dev).reshape(-1, 1, 1) if not isinstance(norm["mean"], float) else norm["mean"]
    std = torch.tensor(norm["std"], device=dev).reshape(-1, 1, 1) if not isinstance(norm["std"], float) else norm["std"]

    def arm_a():
        return eng.rollout_eval(x, y, param=param, **norm)[:2]

    def arm_b():
        return eng.rollout_eval_spectrum(x, y, param=param, **norm)

    def arm_c():
        return eng.rollout_eval_spectrum(x, y, param=param, spectrum_steps=every8, **norm)

    def torch_spectra(u):
        """u [B, t, C, H, W] denormalised -> [B, t, C, S]"""
        F = torch.fft.rfft2(u) / float(H * W)
        p = ((F.real ** 2 + F.imag ** 2) * wgt).reshape(u.shape[:3] + (-1,))
        return torch.zeros(u.shape[:3] + (S,), device=dev).index_add_(3, idx, p)

    def arm_d():
        out = eng.rollout(x, T, param=param)
        f, s = metrics.relative_l2(out, y, **norm)
        spectra = torch.empty((B, T, C, 3, S), device=dev)
        for t0 in range(0, T, 16):                                # the transform's complex planes, 16 steps at a time
            p, q = out[:, t0:t0 + 16] * std + mean, y[:, t0:t0 + 16] * std + mean
            for k, u in enumerate((p, q, p - q)):
                spectra[:, t0:t0 + 16, :, k] = torch_spectra(u)
        return f, s, spectra

    if a.only_b:
        for _ in range(a.only_b):
            arm_b()
        torch.cuda.synchronize()
        return

    arms = {"a": arm_a, "b": arm_b, "c": arm_c}
    note_d = None
    try:
        rd = arm_d()
        torch.cuda.synchronize()
        arms["d"] = arm_d
    except Exception as ex:  # noqa: BLE001
        note_d = "arm (d) left out: torch.fft is not usable on this box (%s: %s)" % (type(ex).__name__, str(ex)[:200])
        rd = None

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
    ra, rb = arm_a(), arm_b()
    torch.cuda.synchronize()
    same = all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(ra, (rb.frame, rb.seq)))
    agree = None
    if rd is not None:                                            # (d) is another algorithm: agreement, not equality
        e64 = rd[2].double()
        bound = 2e-5 * e64 + 2e-7 * e64.sum(-1, keepdim=True)
        agree = float(((rb.spectra.double() - e64).abs() / bound).max())
    del ra, rb, rd
    times = {k: [] for k in arms}
    for _ in range(a.blocks):
        for k, fn in arms.items():
            times[k].append(block(fn))
    med = {k: statistics.median(v) for k, v in times.items()}
    peaks = {k: peak(fn) for k, fn in arms.items()}
    res = dict(
        tool="eval_spectrum_time", preset=a.preset, batch=B, rollout=T, blocks=a.blocks, calls_per_block=a.calls, warmup=a.warmup,
        device=torch.cuda.get_device_name(dev), bins=S,
        ms_per_call={k: round(v, 3) for k, v in med.items()}, ms_per_call_blocks={k: [round(t, 3) for t in v] for k, v in times.items()},
        a_block_spread=round((max(times["a"]) - min(times["a"])) / med["a"], 4),
        b_over_a=round(med["b"] / med["a"], 4), c_over_a=round(med["c"] / med["a"], 4),
        d_over_b=round(med["d"] / med["b"], 4) if "d" in med else None,
        peak_bytes_above_resident=peaks, rollout_tensor_bytes=B * T * C * H * W * 4,
        frame_seq_bitwise_equal_a_b=bool(same), b_against_d_worst_ratio_to_test_bound=agree, note=note_d)
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

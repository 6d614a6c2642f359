"""Validation step with energy spectra under two bases, on one box and in one process (default options, arms interleaved):
  (a) Engine.rollout_eval                                   -- the streaming validation without spectra: the yardstick
  (b) Engine.rollout_eval_spectrum, every step, dft / dft   -- the spectra as they were
  (c) Engine.rollout_eval_spectrum, every step, dct / dct   -- a DCT-II on both axes
Warm-up, then `blocks` synchronised blocks of `calls` calls per arm; the figure of an arm is the median over its blocks of
(block time / calls), (b)'s spread is (max - min) / median over its blocks: (c) / (b) is to be read against it.  The result
is merged into a JSON file under the key "T<rollout>".  No gate: nothing was promised for the DCT path.

    python tools/eval_spectrum_basis_time.py [--preset ns2d_128] [--batch 64] [--rollout 64] [--out profiles/rollout_eval_spectrum_basis_time.json]
    rocprofv3 --kernel-trace --stats -d out -- python tools/eval_spectrum_basis_time.py --only-c 3      # arm (c) alone, for a kernel trace
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="ns2d_128")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rollout", type=int, default=64)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--basis", default="dct", help='arm (c): "dct", or "y,x" such as "dct,dft"')
    ap.add_argument("--only-c", type=int, default=0, help="run arm (c) this many times and nothing else (kernel traces)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_eval_spectrum_basis_time.json"))
    a = ap.parse_args()
    B, T = a.batch, a.rollout
    basis = tuple(a.basis.split(",")) if "," in a.basis else a.basis
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

    def arm_a():
        return eng.rollout_eval(x, y, param=param, **norm)[:2]

    def arm_b():
        return eng.rollout_eval_spectrum(x, y, param=param, **norm)

    def arm_c():
        return eng.rollout_eval_spectrum(x, y, param=param, basis=basis, **norm)

    if a.only_c:
        for _ in range(a.only_c):
            arm_c()
        torch.cuda.synchronize()
        return

    arms = {"a": arm_a, "b": arm_b, "c": arm_c}

    def block(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.calls):
            r = fn()
        torch.cuda.synchronize()
        del r
        return (time.perf_counter() - t0) * 1e3 / a.calls

    for _ in range(a.warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    ra, rb, rc = arm_a(), arm_b(), arm_c()
    torch.cuda.synchronize()
    same = all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for r in (rb, rc) for p, q in zip(ra, (r.frame, r.seq)))
    # Parseval ties the two bases together: the bins of a row sum to mean(u^2) under either
    parseval = float(((rb.spectra.double().sum(-1) - rc.spectra.double().sum(-1)).abs() / rb.spectra.double().sum(-1)).max())
    bins = {"b": int(rb.spectra.shape[-1]), "c": int(rc.spectra.shape[-1])}
    del ra, rb, rc
    times = {k: [] for k in arms}
    for _ in range(a.blocks):
        for k, fn in arms.items():
            times[k].append(block(fn))
    med = {k: statistics.median(v) for k, v in times.items()}
    res = dict(
        tool="eval_spectrum_basis_time", preset=a.preset, batch=B, rollout=T, blocks=a.blocks, calls_per_block=a.calls,
        warmup=a.warmup, device=torch.cuda.get_device_name(dev), basis_c=list(eng._basis_names(basis)), bins=bins,
        wavenumber_step_c=float(metrics.spectrum_wavenumbers(H, W, eng._basis_names(basis))[1]),
        ms_per_call={k: round(v, 3) for k, v in med.items()}, ms_per_call_blocks={k: [round(t, 3) for t in v] for k, v in times.items()},
        b_block_spread=round((max(times["b"]) - min(times["b"])) / med["b"], 4),
        b_over_a=round(med["b"] / med["a"], 4), c_over_a=round(med["c"] / med["a"], 4), c_over_b=round(med["c"] / med["b"], 4),
        frame_seq_bitwise_equal_a_b_c=bool(same), row_sums_b_against_c_worst_relative=parseval)
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

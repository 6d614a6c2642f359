"""Slice rule of the batch-parallel weight gradient (csrc/wgrad_split.inc: WG_TARGET_BLOCKS, WG_MAX_SLICES): the whole
training step of the four recorded shapes (tools/train_time.py) under a few values of the two constants, set through the
tuning knobs LNS_WGRAD_TARGET_BLOCKS / LNS_WGRAD_MAX_SLICES, which the library reads once per process: one child process
per setting and shape.  Per setting: median of `--blocks` blocks of `--block` steps.

    python tools/wgrad_sweep.py [--out profiles/wgrad_split_slices.txt]
"""
import argparse
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import train_time as tt  # noqa: E402

SETTINGS = ((64, 128), (128, 128), (256, 128), (512, 128), (1024, 128), (512, 32), (1024, 256))   # (target blocks, max slices)


def time_arm(preset, T, dev, wgrad, a):
    arms, _ = tt.arms_for(preset, T, dev, only=("trainer_split" if wgrad == "split" else "trainer",))
    step = next(iter(arms.values()))
    for _ in range(a.warmup):
        step()
    return statistics.median(tt.block_ms(step, a.block) for _ in range(a.blocks)) / a.block


def child(preset, T, wgrad, a, env):
    """step_ms of one arm in a fresh process (the knobs are read once per process)"""
    cmd = [sys.executable, os.path.abspath(__file__), "--child", preset, str(T), wgrad, "--blocks", str(a.blocks), "--block", str(a.block),
           "--warmup", str(a.warmup)]
    out = subprocess.run(cmd, env=dict(os.environ, **env), check=True, capture_output=True, text=True, timeout=300).stdout
    return float(out.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--block", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs=3, default=None, metavar=("PRESET", "T", "WGRAD"), help="internal: time one arm and print step_ms")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    if a.child:
        print("%.4f" % time_arm(a.child[0], int(a.child[1]), dev, a.child[2], a))
        return
    lines = ["# step_ms of Stage2Trainer.step, B = %d; 'tile' = option train_wgrad 0; other columns: train_wgrad 1 with" % tt.B,
             "# (WG_TARGET_BLOCKS, WG_MAX_SLICES) = the column head.  %s, torch %s" % (torch.cuda.get_device_name(dev), torch.__version__),
             "%-18s %9s " % ("preset", "tile") + " ".join("%10s" % ("%d/%d" % s) for s in SETTINGS)]
    for preset, T in tt.SHAPES:
        row = ["%9.3f" % child(preset, T, "tile", a, {})]
        for target, smax in SETTINGS:
            row.append("%10.3f" % child(preset, T, "split", a, {"LNS_WGRAD_TARGET_BLOCKS": str(target), "LNS_WGRAD_MAX_SLICES": str(smax)}))
        lines.append("%-18s " % preset + " ".join(row))
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

"""What a tangent step costs beside the forward it linearises, on one box and in one process (synthetic latents, B = 8, T = 8,
the `ns2d_128` and `twophase_cond` latents):
  (a)  Engine.train_forward at batch B: the yardstick
  (b)  train_forward at batch B + train_tangent for K = 1, 4, 16 tangents per sample (no stored steps)
  (c)  train_forward at batch B * K: what carrying K perturbations by differencing nonlinear rollouts would cost
Warm-up, then blocks of `--block` calls with one synchronisation before and after each block, the arms interleaved block by
block; per arm the median block time and its min / max, (b) / (a) and (b) / (c) beside (a)'s own block spread.  Workspaces are
allocated once, outside the timed blocks.

    python tools/tangent_time.py [--blocks 5] [--block 10] [--warmup 1] [--out profiles/rollout_tangent_time.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/tangent_time.py --trace-arm 4 --shape ns2d_128
    python tools/tangent_time.py --kernel-stats DIR/<host>/<pid>_kernel_stats.csv profiles/rollout_tangent_time.json ns2d_128/K4

--trace-arm K runs arm (b) for K on its own, with one lns_op_orthonormalize per call (what a Lyapunov loop with renorm = T
adds), for a kernel trace; --kernel-stats (host only) merges the new kernels' rows of that trace into the record.

What a run does not show: wall time of a block, not GPU kernel time (the kernel shares come from the trace); (b) without stored
steps -- jv_out adds one strided copy of [B*K, c, h, w] per step; nothing about accuracy (tools/tangent_parity.py).
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

B, T, KS = 8, 8, (1, 4, 16)
PRESETS = ("ns2d_128", "twophase_cond")
NEW_KERNELS = ("gn_train_jvp_kernel", "gelu_jvp_kernel", "chan_scale_rows_kernel", "orthonormalize_kernel")


def arms_for(preset, dev, ks=KS, orth=False):
    from lns_amd import engine, filler, tangent
    import train_time
    _, model = train_time.build(preset, dev)
    eng = model._eng
    eng.set_option("train_wgrad", 0)
    c, h, w = eng.latent_shape()
    roll = tangent.TangentRollout(model)
    roll._current()
    arr = roll._arr

    def latent(n, name):
        return torch.from_numpy(filler.normal(name, (n, c, h, w), 11) * 0.5).to(dev)

    def param(n):
        return torch.from_numpy(filler.uniform01("param", n, 11).astype("float32")).to(dev) if model._conditional else None
    z, p = latent(B, "z_in"), param(B)
    ws_a = torch.empty(eng.train_tangent_workspace_bytes(B, h, w, T, 1), dtype=torch.uint8, device=dev)
    arms = {"a_forward_B": lambda n: [eng.train_forward(arr, z, T, param=p, workspace=ws_a) for _ in range(n)]}
    for K in ks:
        v = latent(B * K, "v").reshape(B, K, c, h, w)
        ws = torch.empty(eng.train_tangent_workspace_bytes(B, h, w, T, K), dtype=torch.uint8, device=dev)

        def b_arm(n, v=v, ws=ws):
            for _ in range(n):
                eng.train_forward(arr, z, T, param=p, workspace=ws)
                eng.train_tangent(arr, v, T, ws)
                if orth:
                    engine.orthonormalize(v)
        arms["b_forward_tangent_K%d" % K] = b_arm
        if not orth:
            zk, pk = latent(B * K, "z_in"), param(B * K)
            wsk = torch.empty(eng.train_tangent_workspace_bytes(B * K, h, w, T, 1), dtype=torch.uint8, device=dev)
            arms["c_forward_BK_K%d" % K] = lambda n, zk=zk, pk=pk, wsk=wsk: [eng.train_forward(arr, zk, T, param=pk, workspace=wsk) for _ in range(n)]
    return arms, (c, h, w)


def kernel_stats(stats_csv, out_json, label):
    """rocprofv3's <pid>_kernel_stats.csv -> the rows of the new kernels and the total, merged into the record under `label`."""
    import csv
    rows, total = {}, 0.0
    with open(stats_csv) as f:
        for row in csv.DictReader(f):
            ns = float(row["TotalDurationNs"])
            total += ns
            for k in NEW_KERNELS:
                if k in row["Name"]:
                    rows[k] = dict(calls=int(row["Calls"]), total_us=round(ns / 1e3, 1), average_us=round(float(row["AverageNs"]) / 1e3, 2))
    for k in rows:
        rows[k]["share_of_kernel_time"] = round(rows[k]["total_us"] * 1e3 / total, 4)
    doc = json.load(open(out_json)) if os.path.exists(out_json) else {}
    doc.setdefault("kernel_trace", {})[label] = dict(
        source="rocprofv3 --kernel-trace --stats, arm (b) with one orthonormalisation per call, a run of its own (the weight packs' "
               "kernels included)", all_kernels_total_us=round(total / 1e3, 1), kernels=rows)
    print(json.dumps(doc["kernel_trace"][label]))
    with open(out_json, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--block", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-arm", type=int, default=0, metavar="K", help="run arm (b) for K with an orthonormalisation, and nothing else")
    ap.add_argument("--shape", default=PRESETS[0])
    ap.add_argument("--kernel-stats", nargs=3, metavar=("KERNEL_STATS_CSV", "RECORD_JSON", "LABEL"))
    a = ap.parse_args()
    if a.kernel_stats:
        return kernel_stats(*a.kernel_stats)
    dev = torch.device("cuda:0")
    if a.trace_arm:
        arms, _ = arms_for(a.shape, dev, ks=(a.trace_arm,), orth=True)
        arms["b_forward_tangent_K%d" % a.trace_arm](a.block)
        torch.cuda.synchronize()
        return
    rec = {"B": B, "T": T, "K": list(KS), "block": a.block, "blocks": a.blocks, "device": torch.cuda.get_device_name(0), "shapes": {}}
    for preset in PRESETS:
        arms, latent = arms_for(preset, dev)
        for run in arms.values():
            for _ in range(a.warmup):
                run(a.block)
        torch.cuda.synchronize()
        times = {k: [] for k in arms}
        for _ in range(a.blocks):
            for k, run in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(a.block)
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) / a.block * 1e3)
        row = {"latent": list(latent)}
        for k, v in times.items():
            row[k] = {"ms_per_call_median": statistics.median(v), "min": min(v), "max": max(v)}
        fa = row["a_forward_B"]
        row["a_block_spread_max_over_min"] = fa["max"] / fa["min"]
        for K in KS:
            b = row["b_forward_tangent_K%d" % K]["ms_per_call_median"]
            row["b_over_a_K%d" % K] = b / fa["ms_per_call_median"]
            row["b_over_c_K%d" % K] = b / row["c_forward_BK_K%d" % K]["ms_per_call_median"]
            row["tangent_over_c_K%d" % K] = (b - fa["ms_per_call_median"]) / row["c_forward_BK_K%d" % K]["ms_per_call_median"]
        rec["shapes"][preset] = row
        print(preset, json.dumps(row))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The float32 CPU oracle against the float64 statements of tests/fa_axis_reference.py on every reducer and low-rank-kernel
input set of tests/test_fa_axis_gpu.py: the oracle's relative L2 error (worst sample, or worst (sample, head)) and the
tolerance the GPU test holds the kernels to -- KERNEL_TOL, or TOL_FACTOR times the oracle's error for the offset-row reducer
sets and the low-rank-kernel sets.  Needs no GPU.

    python tools/fa_axis_parity.py [--out profiles/fa_axis_parity.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import fa_axis_reference as fr  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fa_axis_parity.json"))
    out = ap.parse_args().out
    sets = {}
    for kernel, rows in (("reducer", [fr.reducer_set(*s) for s in fr.reducer_sets()]), ("lrk", [fr.lrk_set(*s) for s in fr.lrk_sets()])):
        for r in rows:
            sets[r["name"]] = dict(kernel=kernel, per="sample" if kernel == "reducer" else "(sample, head)",
                                   oracle_err=float(r["oracle_err"].max()), tolerance=float(r["tol"]),
                                   rule="KERNEL_TOL" if r["tol"] == fr.KERNEL_TOL else "TOL_FACTOR x oracle_err")
    rec = dict(kernel_tol=fr.KERNEL_TOL, oracle_tol=fr.ORACLE_TOL, tol_factor=fr.TOL_FACTOR, sets=sets)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    for n, e in sets.items():
        print("%-36s oracle %.2e  tolerance %.2e  (%s)" % (n, e["oracle_err"], e["tolerance"], e["rule"]))


if __name__ == "__main__":
    main()

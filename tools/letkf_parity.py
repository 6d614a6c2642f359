"""The patch Gram of the localised ensemble Kalman filter against its numpy statement (tests/letkf_reference.py), as a record: per
case of tests/test_letkf_gpu.py (M x plane x latent grid) the device's worst ratio to the bound max(1e-12, 3 x the float64
statement's own distance from its longdouble form) over G, g and stat of every patch.  The cases, the bound and the assertions are
the tests': this tool runs them and writes what they measured.  A ratio of 1 / 3 means that the device gave the float64
statement's bits on the case that decides.  (Combine and the update are held bit for bit by the tests; there is no ratio to record.)

    python tools/letkf_parity.py [--out profiles/letkf_parity.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import test_letkf_gpu as tg  # noqa: E402


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "letkf_parity.json"))
    a = ap.parse_args()
    for m in (2, 3, 7, 33, 64):
        for hw, grid in tg.PLANE_GRIDS:
            tg.test_patch_gram_op_under_the_rule(m, hw, grid)
    ratios = dict(tg.RATIOS)
    rec = dict(tool="letkf_parity", device=torch.cuda.get_device_name(0), rule="max(1e-12, 3 x own) in rel-L2 and in max|diff| / max|ref|",
               worst_ratio_to_the_bound=ratios, worst_of_all=max(ratios.values()))
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

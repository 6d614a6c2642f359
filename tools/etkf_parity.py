"""The ensemble transform Kalman filter against its numpy statement (tests/etkf_reference.py), as a record: per case of
tests/test_etkf_gpu.py the device's worst ratio to the bound max(1e-12, 3 x the float64 statement's own distance from its
longdouble form) over S, g, stat (the Gram op, M x plane) and over X, wbar, lam and the residual || W A W - (M - 1) I || (the
transform op, per M, cond(A) 1 .. 1e4), and the twin experiment's analysis / forecast misfit per sample on the device beside the
float64 reference's through the CPU oracle.  The cases, the bound and the assertions are the tests': this tool runs them and
writes what they measured.  A ratio of 1 / 3 means that the device gave the float64 statement's bits on the case that decides.

    python tools/etkf_parity.py [--out profiles/etkf_parity.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import etkf_reference as er  # noqa: E402
import test_etkf_gpu as tg  # noqa: E402


def reference_twin():
    """tests/test_etkf_cpu.py's twin experiment -> the float64 reference's analysis / forecast misfit per sample"""
    import io
    import re
    from contextlib import redirect_stdout
    import test_etkf_cpu as tc
    buf = io.StringIO()
    with redirect_stdout(buf):
        tc.test_twin_experiment_through_the_oracle_halves_the_misfit()
    return [float(v) for v in re.findall(r"[0-9.]+", buf.getvalue().split("per sample")[1])]


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "etkf_parity.json"))
    a = ap.parse_args()
    for m in (2, 3, 7, 33, 64):
        for hw in tg.PLANES:
            tg.test_gram_op_under_the_rule(m, hw)
        tg.test_transform_op_under_the_rule(m)
    tg.test_twin_experiment_through_assimilate_ensemble()
    ratios = dict(tg.RATIOS)
    twin = ratios.pop("twin analysis/forecast misfit")
    rec = dict(tool="etkf_parity", device=torch.cuda.get_device_name(0), rule="max(1e-12, 3 x own) in rel-L2 and in max|diff| / max|ref|",
               worst_ratio_to_the_bound=ratios, worst_of_all=max(ratios.values()),
               twin=dict(settings=er.TWIN, reference_float64_analysis_over_forecast=reference_twin(), device_analysis_over_forecast=twin,
                         note="the device draws its own noise (torch generator), the reference numpy's: two draws of one experiment; "
                              "over the numpy seeds 1 .. 30 the reference's factor ranged 0.22 .. 0.87"))
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

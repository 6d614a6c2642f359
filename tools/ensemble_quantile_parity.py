"""How close are the ensemble quantiles to float64?  The cases of tests/test_ensemble_quantile_gpu.py::
test_op_quantiles_against_float64 (its families and member counts, through its own helpers): lns_op_ensemble_quantiles against
numpy.quantile(method="linear") in float64 on the same fp32 inputs, under the project's rule max(2e-7, 3 x own) in
max |diff| / max |ref| and in rel-L2 per output tensor, `own` being torch.quantile's fp32 distance from the same float64
values.  Writes, per family, the worst ratio ours / bound over the member counts in either measure, the errors behind it, and
whether every probability equalled the float64 count over M rounded to fp32.

    python tools/ensemble_quantile_parity.py [--out profiles/ensemble_quantile_parity.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_quantile_parity.json"))
    a = ap.parse_args()
    import torch
    import ensemble_quantile_reference as ref
    import test_ensemble_quantile_gpu as t
    rec = dict(tool="ensemble_quantile_parity", device=torch.cuda.get_device_name(0), rule="max(2e-7, 3 x own)",
               probabilities=list(t.PROBS), members=[2, 7, 33, 128], shape="B=2 n=2 C=3 23x29", families={})
    for m in rec["members"]:
        g = torch.Generator(device="cuda")
        g.manual_seed(400 + m)
        for name, frames, thr in t.float64_families(m, g):
            quant, prob = t._op(frames, t.PROBS, thr, None)
            q64, p64 = ref.quantiles64(frames, t.PROBS, thr)
            own, _ = ref.own32(frames, t.PROBS, thr)
            want = q64.cuda()

            def errs(x):
                d = x.double() - want
                return float(d.abs().max() / want.abs().max()), float(d.norm() / want.norm())
            o, w = errs(quant), errs(own)
            ratios = [x / max(t.FLOOR, 3.0 * y) for x, y in zip(o, w)]
            f = rec["families"].setdefault(name, dict(worst_ratio=0.0, prob_exact=True, per_members={}))
            f["per_members"]["M=%d" % m] = dict(ours_rel_max=o[0], own_rel_max=w[0], ours_rel_l2=o[1], own_rel_l2=w[1],
                                                ratio_rel_max=round(ratios[0], 4), ratio_rel_l2=round(ratios[1], 4))
            f["worst_ratio"] = max(f["worst_ratio"], round(max(ratios), 4))
            f["prob_exact"] = f["prob_exact"] and bool(torch.equal(prob.cpu(), p64.float()))
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

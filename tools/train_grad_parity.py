"""The shape grid of tests/test_train_grad_shapes_gpu.py outside pytest: every (engine, B, T, h, w) case of
tests/train_reference.py, both weight-gradient forms (option "train_wgrad" 0 / 1), the HIP training rollout against the
float64 autograd reference on the CPU.  Per case and form the record holds the worst tensor (largest error / bound in
either measure), its engine error, `own` (the float32 CPU run of the reference against its float64 run) and their ratio,
in both measures (rel-L2 and max |diff| / max |ref|), plus the loss and z_pred errors.

    python tools/train_grad_parity.py [--out profiles/train_grad_shapes.json] [--only E1]

Stops at the first case the engine cannot run (an error from a training call is recorded with its message and ends the
run: nothing more is started on the device after it).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

import train_reference as tr  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_grad_shapes.json"))
    ap.add_argument("--only", default=None, help="engine name (E1 .. E7)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    rec = dict(tool="tools/train_grad_parity.py", device=torch.cuda.get_device_name(0), grad_tol=tr.GRAD_TOL,
               rule="error <= max(grad_tol, 3 * own) per tensor, in rel-L2 and in max|diff|/max|ref|",
               weight_seed=tr.WEIGHT_SEED, input_seed=tr.INPUT_SEED, z_scale=tr.Z_SCALE,
               engines={k: {f: v[f] for f in ("family", "c", "D", "blocks", "dilation")} for k, v in tr.ENGINES.items()},
               cases=[])
    ok = True
    for case in tr.CASES:
        if a.only and case[0] != a.only:
            continue
        for form in tr.FORMS:
            t0 = time.time()
            row = dict(case=tr.case_id(case), engine=case[0], B=case[1], T=case[2], h=case[3], w=case[4], train_wgrad=form)
            try:
                rows, dloss, loss, ezp = tr.compare(case, form)
            except Exception as ex:  # noqa: BLE001 -- recorded, and the run ends here
                row["error"] = "%s: %s" % (type(ex).__name__, ex)
                rec["cases"].append(row)
                ok = False
                break
            k, e2, b2, em, bm, o2, om = max(rows, key=lambda r: max(r[1] / r[2], r[3] / r[4]))
            passed = all(r[1] <= r[2] and r[3] <= r[4] for r in rows) and dloss <= 2e-6 * abs(loss) + 1e-7 and ezp < 2e-5
            row.update(worst_tensor=k, rel_l2=e2, own_rel_l2=o2, rel_l2_over_own=e2 / o2 if o2 > 0 else None, rel_l2_bound=b2,
                       rel_max=em, own_rel_max=om, rel_max_over_own=em / om if om > 0 else None, rel_max_bound=bm,
                       loss=loss, loss_abs_err=dloss, z_pred_rel_l2=ezp, tensors=len(rows), passed=bool(passed),
                       seconds=round(time.time() - t0, 2))
            ok = ok and passed
            rec["cases"].append(row)
            print("%-22s form %d  %-44s rel-L2 %.2e (own %.2e)  rel-max %.2e (own %.2e)  z_pred %.2e  %s"
                  % (row["case"], form, k, e2, o2, em, om, ezp, "ok" if passed else "FAIL"), flush=True)
        if not ok and "error" in rec["cases"][-1]:
            break
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", a.out)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

"""The Gauss-Newton latent fit against its float64 statement (tests/latent_fit_gn_reference.py), as a record:
  * per case of the adjoint grid, per weight-gradient form, with and without background / damping: ours / bound of H v and
    v^T H v (lns_train_gn_product) in rel-L2 and rel-max, the bound being max(GRAD_TOL, 3 x the float32 statement's own error),
    and the symmetry defect |<u, H v> - <v, H u>| / (|sqrt(W) J u| |sqrt(W) J v|);
  * per twin experiment (param known): worst-sample loss[0] / loss[-1] of LatentFit.run_gauss_newton after 1 x 8 and 3 x 8
    beside the float64 statement's, the loss sequences, and the state error against the truth relative to the start's.

    python tools/latent_fit_gn_parity.py [--out profiles/latent_fit_gn_parity.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import latent_fit_gn_reference as gn  # noqa: E402
import latent_fit_reference as lf  # noqa: E402
import train_reference as tr  # noqa: E402
from lns_amd import fit  # noqa: E402


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda() if a is not None else None


def product(case, form, lam, mu):
    name, B, T, h, w = case
    model = tr.grid_model(name)
    eng = model._owner._eng
    eng.set_option("train_wgrad", form)
    z0, prm, v, u = gn.case_start(case)
    steps, wts = gn.case_obs(case)
    params = {k: p.detach() for k, p in model.named_parameters() if k.startswith("propagator.")}
    z0, p, v, u = cuda(z0), cuda(prm), cuda(v), cuda(u)
    ws = torch.empty(eng.train_gn_product_workspace_bytes(B, h, w, T, len(steps)), dtype=torch.uint8, device="cuda")
    z_pred, _ = eng.train_forward(params, z0, T, param=p, workspace=ws)
    hv, vhv = eng.train_gn_product(params, z0, z_pred, v, steps, ws, weights=wts, background=lam, damping=mu)
    hu, _ = eng.train_gn_product(params, z0, z_pred, u, steps, ws, weights=wts, background=lam, damping=mu)
    r64, r32 = gn.product_truth(case, lam, mu)
    row = {}
    for k, ours in (("hv", hv), ("vhv", vhv)):
        e2, b2, em, bm, o2, om = lf.rule(ours.cpu().numpy(), r64[k], r32[k])
        row[k] = {"rel_l2": e2, "rel_l2_bound": b2, "rel_max": em, "rel_max_bound": bm, "own_rel_l2": o2, "own_rel_max": om,
                  "worst_over_bound": max(e2 / b2, em / bm)}
    n = v[0].numel()
    cw = np.array([2.0 * wk / n for wk in wts])
    scale = np.sqrt((cw[None] * (r64["ju"] ** 2).reshape(B, len(cw), -1).sum(2)).sum(1)) * \
        np.sqrt((cw[None] * (r64["jv"] ** 2).reshape(B, len(cw), -1).sum(2)).sum(1))
    u64, v64, hv64, hu64 = (t.double().cpu().reshape(B, -1) for t in (u, v, hv, hu))
    row["symmetry_defect_over_scale"] = float((((u64 * hv64).sum(1) - (v64 * hu64).sum(1)).abs().numpy() / scale).max())
    row["min_vhv"] = float(vhv.min())
    return row


def twin(setup):
    d = lf.twin(setup)
    model = tr.grid_model(setup[0])
    model._owner._eng.set_option("train_wgrad", 0)
    B = setup[1]
    row = {}
    err = lambda z: np.sqrt(((z - d["z_true"]).astype(np.float64) ** 2).reshape(B, -1).sum(1))      # noqa: E731
    for outer in (1, 3):
        res = fit.LatentFit(model).run_gauss_newton(cuda(d["z_start"]), cuda(d["obs"]), lf.TWIN_STEPS, param=cuda(d["p_true"]),
                                                    weights=lf.TWIN_WEIGHTS, outer=outer, cg_iters=gn.CG_ITERS)
        z64, l64 = gn.twin_fit(setup, outer=outer)
        lg = res.loss.cpu().numpy().astype(np.float64)
        row["%dx%d" % (outer, gn.CG_ITERS)] = {
            "loss_engine": lg.tolist(), "loss_float64": l64.numpy().tolist(),
            "reduction_engine": (lg[0] / lg[-1]).tolist(), "reduction_float64": (l64[0] / l64[-1]).tolist(),
            "recorded_worst_sample": gn.MEASURED[(outer, gn.CG_ITERS)][setup], "gpu_gate": gn.GPU_FRACTION * gn.MEASURED[(outer, gn.CG_ITERS)][setup],
            "monotone": bool((np.diff(lg, axis=0) <= 0).all()),
            "state_error_over_start": {"engine": (err(res.z0.cpu().numpy()) / err(d["z_start"])).tolist(),
                                       "float64": (err(z64.numpy()) / err(d["z_start"])).tolist()}}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rec = {"device": torch.cuda.get_device_name(0), "grad_tol": tr.GRAD_TOL, "product": {}, "twin": {}}
    for case in lf.ADJOINT_CASES:
        for form in tr.FORMS:
            for lam, mu in ((0.0, 0.0), (gn.GN_LAMBDA, gn.GN_DAMPING)):
                rec["product"]["%s/train_wgrad=%d/background=%g/damping=%g" % (tr.case_id(case), form, lam, mu)] = product(case, form, lam, mu)
    for setup in lf.TWINS:
        rec["twin"][tr.case_id(setup)] = twin(setup)
    rec["worst_over_bound"] = max(v["worst_over_bound"] for row in rec["product"].values() for v in row.values()
                                  if isinstance(v, dict) and "worst_over_bound" in v)
    rec["worst_symmetry_defect_over_scale"] = max(row["symmetry_defect_over_scale"] for row in rec["product"].values())
    print(json.dumps(rec, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

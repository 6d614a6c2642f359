"""The latent fit against its float64 statement (tests/latent_fit_reference.py), as a record:
  * per case of the adjoint grid and per weight-gradient form: ours / bound of grad_z0 and grad_param (state-only adjoint) in
    rel-L2 and rel-max, the bound being max(GRAD_TOL, 3 x the float32 statement's own error);
  * per twin experiment: ours / bound of g_z, g_p, per and loss of one lns_fit_step from the start, and after 40 iterations of
    lns_amd.fit.LatentFit the loss and param-error reductions beside the float64 statement's.

    python tools/latent_fit_parity.py [--out profiles/latent_fit_parity.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import latent_fit_reference as lf  # noqa: E402
import train_reference as tr  # noqa: E402
from lns_amd import engine, fit  # noqa: E402


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda() if a is not None else None


def adjoint(case, form):
    name, B, T, h, w = case
    model = tr.grid_model(name)
    eng = model._owner._eng
    eng.set_option("train_wgrad", form)
    _, z_in, z_out, prm = tr.case_inputs(case)
    params = {k: p.detach() for k, p in model.named_parameters() if k.startswith("propagator.")}
    z0, zo, p = cuda(z_in[:, 0].copy()), cuda(z_out), cuda(prm)
    z_pred, ws = eng.train_forward(params, z0, T, param=p)
    zp = z_pred.clone().requires_grad_(True)
    F.smooth_l1_loss(zp, zo).backward()
    out = eng.train_backward(params, z0, z_pred, zp.grad.contiguous(), ws, need_z_grad=True, need_param_grad=p is not None, state_only=True)
    r64, r32 = lf.adjoint_truth(case)
    row = {}
    for k, ours in (("grad_z0", out[1]), ("grad_param", out[2] if p is not None else None)):
        if ours is not None:
            e2, b2, em, bm, o2, om = lf.rule(ours.cpu().numpy(), r64[k], r32[k])
            row[k] = {"rel_l2": e2, "rel_l2_bound": b2, "rel_max": em, "rel_max_bound": bm, "own_rel_l2": o2, "own_rel_max": om,
                      "worst_over_bound": max(e2 / b2, em / bm)}
    return row


def twin(setup):
    d = lf.twin(setup)
    model = tr.grid_model(setup[0])
    eng = model._owner._eng
    eng.set_option("train_wgrad", 0)
    cond = d["p_start"] is not None
    params = {k: p.detach() for k, p in model.named_parameters() if k.startswith("propagator.")}
    z, p, obs = cuda(d["z_start"]), cuda(d["p_start"]), cuda(d["obs"])
    bufs = [torch.zeros_like(z) for _ in range(3)] + ([torch.zeros_like(p) for _ in range(3)] if cond else [None] * 3)
    spec = engine.fit_spec(lf.TWIN_STEPS, lf.TWIN_WEIGHTS, 0.0, state=engine.update_spec(lf.LR_STATE),
                           param=engine.update_spec(lf.LR_PARAM) if cond else None)
    loss, per = eng.fit_step(params, z, obs, spec, param=p, g_z=bufs[0], exp_avg_z=bufs[1], exp_avg_sq_z=bufs[2], g_p=bufs[3],
                             exp_avg_p=bufs[4], exp_avg_sq_p=bufs[5])
    refs = []
    for dt in (torch.float64, torch.float32):
        to = lambda a: torch.from_numpy(a).to(dt) if a is not None else None      # noqa: E731
        refs.append(lf.fit_grads(lf.propagator(setup[0], dt), to(d["z_start"]), to(d["p_start"]), to(d["obs"]), lf.TWIN_STEPS, lf.TWIN_WEIGHTS))
    r64, r32 = refs
    row = {}
    for k, ours in (("g_z", bufs[0]), ("g_p", bufs[3]), ("per", per), ("loss", loss)):
        if ours is not None:
            e2, b2, em, bm, o2, om = lf.rule(ours.cpu().numpy(), r64[k].numpy(), r32[k].double().numpy())
            row[k] = {"rel_l2": e2, "rel_l2_bound": b2, "rel_max": em, "rel_max_bound": bm, "worst_over_bound": max(e2 / b2, em / bm)}
    res = fit.LatentFit(model, lr_state=lf.LR_STATE, lr_param=lf.LR_PARAM).run(cuda(d["z_start"]), obs, lf.TWIN_STEPS, param=cuda(d["p_start"]),
                                                                               weights=lf.TWIN_WEIGHTS, iters=lf.TWIN_ITERS)
    z64, p64, l64 = lf.fit(lf.propagator(setup[0]), lf.t64(d["z_start"]), lf.t64(d["p_start"]), lf.t64(d["obs"]), lf.TWIN_STEPS, lf.TWIN_WEIGHTS)
    lg = res.loss.cpu().numpy()
    row["loss_reduction"] = {"engine": (lg[0] / lg[-1]).tolist(), "float64": (l64[0] / l64[-1]).tolist()}
    if cond:
        row["param_error"] = {"start": lf.PARAM_OFFSET, "engine": np.abs(res.param.cpu().numpy() - d["p_true"]).tolist(),
                              "float64": np.abs(p64.numpy() - d["p_true"]).tolist()}
    rms = lambda a: np.sqrt(((a - d["z_true"]) ** 2).reshape(setup[1], -1).mean(1)).tolist()      # noqa: E731
    row["rms_state_error"] = {"start": rms(d["z_start"]), "engine": rms(res.z0.cpu().numpy()), "float64": rms(z64.numpy())}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rec = {"device": torch.cuda.get_device_name(0), "grad_tol": tr.GRAD_TOL, "adjoint": {}, "twin": {}}
    for case in lf.ADJOINT_CASES:
        for form in tr.FORMS:
            rec["adjoint"]["%s/train_wgrad=%d" % (tr.case_id(case), form)] = adjoint(case, form)
    for setup in lf.TWINS:
        rec["twin"][tr.case_id(setup)] = twin(setup)
    rec["worst_over_bound"] = max(v["worst_over_bound"] for part in (rec["adjoint"], rec["twin"]) for row in part.values()
                                  for v in row.values() if isinstance(v, dict) and "worst_over_bound" in v)
    print(json.dumps(rec, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

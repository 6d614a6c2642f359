"""The tangent-linear rollout against its float64 statement (tests/tangent_reference.py), as a record:
  * per case of the grid and per weight-gradient form (the workspace layout differs): ours / bound of jv over the stored steps
    in rel-L2 and rel-max, the bound being max(GRAD_TOL, 3 x the float32 statement's own error);
  * per case of the dot-product grid: |<J v, w> - <v, J^T w>| / (|J v| |w|) between lns_train_tangent and the state-only adjoint;
  * lns_op_orthonormalize per shape and input family: the reconstruction error of Q R, Q and log R_kk against the float64
    statement (N(0,1), K <= n / 2), and |Q^T Q - I| beside what the fp32 statement reaches on the same input;
  * the Lyapunov exponents of the test cases beside the float64 and float32 loops from the same start vectors.

    python tools/tangent_parity.py [--out profiles/tangent_parity.json]
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
import latent_fit_reference as lf  # noqa: E402
import tangent_reference as tg  # noqa: E402
import train_reference as tr  # noqa: E402
from lns_amd import engine, filler, tangent  # noqa: E402

ORTH_TOL, SEED = 2e-7, 1234


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda() if a is not None else None


def run(case, K, form):
    name, B, T, h, w = case
    model = tr.grid_model(name)
    eng = model._owner._eng
    eng.set_option("train_wgrad", form)
    z0, prm, v = (cuda(a) for a in tg.case_start(case, K))
    params = {k: p.detach() for k, p in model.named_parameters() if k.startswith("propagator.")}
    ws = torch.empty(eng.train_tangent_workspace_bytes(B, h, w, T, K), dtype=torch.uint8, device="cuda")
    z_pred, _ = eng.train_forward(params, z0, T, param=prm, workspace=ws)
    vv = v.clone()
    jv = eng.train_tangent(params, vv, T, ws, keep=True)
    return eng, params, z0, v, z_pred, ws, jv


def jv_row(case, K, form):
    jv = run(case, K, form)[-1].cpu().numpy()
    r64, r32 = tg.truth(case, K)
    steps = [lf.rule(jv[:, :, s], r64["jv"][:, :, s], r32["jv"][:, :, s]) for s in range(case[2])]
    return {"rel_l2": max(s[0] for s in steps), "rel_l2_bound": min(s[1] for s in steps), "rel_max": max(s[2] for s in steps),
            "rel_max_bound": min(s[3] for s in steps), "own_rel_l2": max(s[4] for s in steps), "own_rel_max": max(s[5] for s in steps),
            "worst_over_bound": max(max(s[0] / s[1], s[2] / s[3]) for s in steps)}


def dot_row(case, K):
    eng, params, z0, v, z_pred, ws, jv = run(case, K, 0)
    B = case[1]
    wv = cuda(filler.normal("tangent_w", tuple(z0.shape), 5))
    g = torch.zeros_like(z_pred)
    g[:, -1] = wv
    _, gz = eng.train_backward(params, z0, z_pred, g, ws, need_z_grad=True, state_only=True)
    jl, w64, v64, g64 = (t.double().cpu() for t in (jv[:, :, -1], wv, v, gz))
    lhs = (jl * w64[:, None]).reshape(B, K, -1).sum(2)
    rhs = (v64 * g64[:, None]).reshape(B, K, -1).sum(2)
    scale = jl.reshape(B, K, -1).norm(dim=2) * w64.reshape(B, 1, -1).norm(dim=2)
    return {"defect": float(((lhs - rhs).abs() / scale).max()), "bound": 2e-4}


def gram(Q):
    Q = np.asarray(Q, np.float64)
    return float(np.abs(np.einsum("bjn,bkn->bjk", Q, Q) - np.eye(Q.shape[1])[None]).max())


def orth_row(shape, family):
    v = tg.orth_input(shape, family)
    q, r = engine.orthonormalize(cuda(v), need_r=True)
    Q, R = q.double().cpu().numpy(), r.cpu().numpy()
    Q32, R32, lr32 = (t.double().numpy() for t in tg.mgs(torch.from_numpy(v), torch.float32))
    rec = lambda Q, R: np.einsum("bjk,bjn->bkn", R, Q)      # noqa: E731
    row = {"qr_rel_l2": tr.rel_l2(rec(Q, R), v), "qr_rel_l2_own": tr.rel_l2(rec(Q32, R32), v), "qr_rel_max": tr.rel_max(rec(Q, R), v),
           "qr_rel_max_own": tr.rel_max(rec(Q32, R32), v), "gram_defect": gram(Q), "gram_defect_fp32_statement": gram(Q32)}
    if family == "normal" and 2 * shape[1] <= shape[2]:
        Q64, _, lr64 = (t.numpy() for t in tg.mgs(torch.from_numpy(v)))
        logr = np.log(np.einsum("bkk->bk", R))
        row.update({"q_rel_l2": tr.rel_l2(Q, Q64), "q_rel_l2_own": tr.rel_l2(Q32, Q64), "logr_rel_l2": tr.rel_l2(logr, lr64),
                    "logr_rel_l2_own": tr.rel_l2(lr32, lr64)})
    return row


def lyapunov_row(case, K, renorm):
    name, B, T, h, w = case
    model = tr.grid_model(name)
    model._owner._eng.set_option("train_wgrad", 0)
    z0, prm, _ = tg.case_start(case, 1)
    gen = lambda: torch.Generator(device="cuda").manual_seed(SEED)      # noqa: E731
    res = tangent.TangentRollout(model).lyapunov(cuda(z0), T, k=K, renorm=renorm, param=cuda(prm), generator=gen())
    V0 = torch.randn((B, K) + z0.shape[1:], dtype=torch.float32, device="cuda", generator=gen()).cpu()
    ref = {}
    for dt in (torch.float64, torch.float32):
        to = lambda a: torch.from_numpy(a).to(dt) if a is not None else None      # noqa: E731
        ref[dt] = tg.lyapunov(lf.propagator(name, dt), to(z0), to(prm), V0.to(dt), T, renorm)[0].double().numpy()
    own = float(np.abs(ref[torch.float32] - ref[torch.float64]).max())
    err = float(np.abs(res.exponents.cpu().numpy() - ref[torch.float64]).max())
    return {"exponents_float64": ref[torch.float64].tolist(), "abs_err": err, "own_abs_err": own, "bound": max(1e-4, 3 * own)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rec = {"device": torch.cuda.get_device_name(0), "grad_tol": tr.GRAD_TOL, "jv": {}, "dot": {}, "orthonormalize": {}, "lyapunov": {}}
    for case, K in tg.GRID:
        for form in tr.FORMS:
            rec["jv"]["%s/train_wgrad=%d" % (tg.grid_id((case, K)), form)] = jv_row(case, K, form)
    for case, K in tg.DOT_GRID:
        rec["dot"][tg.grid_id((case, K))] = dot_row(case, K)
    for shape in tg.ORTH_SHAPES:
        for family in ("normal", "tiny", "huge"):
            rec["orthonormalize"]["%dx%dx%d/%s" % (shape + (family,))] = orth_row(shape, family)
    for case, K, renorm in tg.LYAPUNOV:
        rec["lyapunov"]["%s-K%d-renorm%d" % (tr.case_id(case), K, renorm)] = lyapunov_row(case, K, renorm)
    rec["jv_worst_over_bound"] = max(v["worst_over_bound"] for v in rec["jv"].values())
    rec["gram_defect_worst_over_fp32_statement"] = max(v["gram_defect"] / v["gram_defect_fp32_statement"]
                                                       for v in rec["orthonormalize"].values() if v["gram_defect_fp32_statement"] > 0)
    print(json.dumps(rec, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What do the training walks of the propagator enqueue?  One JSON object: "case/wgradF/call" -> {tensor: first 16 hex digits of
the sha256 of its bytes} for the calls that walk the training tape (csrc/lns_train.inc, csrc/lns_tangent.inc), under option
"train_wgrad" F = 0 and 1:

  train_forward    z_pred
  train_backward   every parameter gradient and grad_z_in for a fixed dL/dz_pred; "state_only/grad_z_in", the state-only
                   adjoint's; on the conditional engine grad_param
  train_tangent    K = 2 tangents through steps t0 = 1 .. 2 (nsteps = 2) with the steps kept: v afterwards and jv_out
  train_step_clip  one clipped step (max_norm below the norm, which the tool asserts): loss, norm, and every parameter, exp_avg
                   and exp_avg_sq after the update
  fit_step         one iteration on observations at steps [0, 2] with a background term, state (and, on the conditional engine,
                   param) fitted: z0, param, loss and per afterwards

Every call runs twice on fresh outputs: a tensor whose two hashes differ (atomics) is left out and named under
"case/wgradF/call/not repeatable".  z_pred, every grad_z_in and the tangent's outputs may not land there (the tool fails).
Two builds that enqueue the same work print the same object.

The cases are engines and planes of tests/train_reference.py (ENGINES / CASES), at B <= 3 and T = 3 (the tangent's window
t0 = 1, nsteps = 2 needs three steps):
  E1-B1-T3-8x8    CASES' own: plain propagator, three blocks, dilation 2
  E1-B3-T3-3x5    CASES' E1-B3-T2-3x5 with a third step: the same engine on a non-square plane smaller than a tile
  E6-B3-T3-7x15   CASES' E6-B5-T2-7x15 with three samples and a third step: conditional propagator, two blocks, dilation 2,
                  non-square

    python tools/train_bits.py [--out FILE]
    python tools/train_bits.py --sizes [--out tests/golden/train_workspace_bytes.json]

--sizes needs no GPU: the five workspace size queries of the training calls over presets x (B, T) x "train_wgrad" x K x n_obs
(SIZE_* below) at each preset's latent plane, the record tests/test_train_layout_cpu.py holds the library to.
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import rollout_bits  # noqa: E402  (sha, dumps)

CASES = (("E1", 1, 3, 8, 8), ("E1", 3, 3, 3, 5), ("E6", 3, 3, 7, 15))
FORMS = (0, 1)
K, T0, NSTEPS = 2, 1, 2
MAX_NORM = 1e-3
OBS_STEPS, BACKGROUND = [0, 2], 0.1
MUST_REPEAT = ("z_pred", "grad_z_in", "state_only/grad_z_in", "v", "jv_out")

SIZE_PRESETS = ("ns2d_mini", "ns2d_64", "twophase_cond", "sw_half_periodic")
SIZE_BT = ((1, 1), (3, 2), (32, 5))
SIZE_K = (1, 5)
SIZE_NOBS = (1, 3)


# ---- workspace sizes (host only) -------------------------------------------------------------------------------------------
def sizes():
    """{"preset/B*_T*/wgrad*": {query: bytes}}: lns_train_workspace_bytes ("train"), lns_train_step_workspace_bytes
    ("train_step"), lns_train_step_clip_workspace_bytes ("train_step_clip"), lns_train_tangent_workspace_bytes ("tangent_K*")
    and lns_fit_step_workspace_bytes ("fit_nobs*")."""
    from lns_amd import config, engine
    rec = {}
    for preset in SIZE_PRESETS:
        a = config.preset(preset)
        e = engine.Engine(engine.make_config(a, ae_prefix="ae." if a.family == "twophase_cond" else "vq_ae.", prop_prefix="propagator."))
        c, h, w = e.latent_shape()
        for form in FORMS:
            e.set_option("train_wgrad", form)
            for B, T in SIZE_BT:
                n = ctypes.c_size_t(0)
                e._check(e._L.lns_train_workspace_bytes(e._h, B, h, w, T, ctypes.byref(n)), "lns_train_workspace_bytes")
                row = {"train": int(n.value), "train_step": e.train_step_workspace_bytes(B, h, w, T),
                       "train_step_clip": e.train_step_clip_workspace_bytes(B, h, w, T)}
                for k in SIZE_K:
                    row["tangent_K%d" % k] = e.train_tangent_workspace_bytes(B, h, w, T, k)
                for n_obs in SIZE_NOBS:
                    row["fit_nobs%d" % n_obs] = e.fit_step_workspace_bytes(B, h, w, T, n_obs)
                rec["%s/B%d_T%d/wgrad%d" % (preset, B, T, form)] = row
    return rec


# ---- bits (GPU) ------------------------------------------------------------------------------------------------------------
def twice(call):
    """call() -> {tensor: hash} on fresh outputs, twice: (what repeats, the names of what does not)."""
    import torch
    runs = []
    for _ in range(2):
        out = call()
        torch.cuda.synchronize()
        runs.append({k: rollout_bits.sha(t) for k, t in out.items()})
    same = {k: v for k, v in runs[0].items() if runs[1][k] == v}
    return same, sorted(set(runs[0]) - set(same))


def case_calls(case):
    """(call name, function returning {tensor name: tensor}) for one case; the engine's option is the caller's."""
    import numpy as np
    import torch
    import train_reference as tr
    from lns_amd import dropin, engine, filler
    name, B, T, h, w = case
    model = dropin.build_dynamics(tr.engine_args(name))
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(v) for k, v in filler.synthetic_state_dict(shapes, tr.WEIGHT_SEED).items()})
    model = model.to("cuda:0")
    eng = model._owner._eng
    c = tr.ENGINES[name]["c"]
    cond = tr.ENGINES[name]["family"] == "twophase_cond"
    params = {k: p.detach() for k, p in model.named_parameters() if k.startswith("propagator.")}

    def normal(tag, shape, scale=0.5):
        return torch.from_numpy(filler.normal(tag, shape, tr.INPUT_SEED) * np.float32(scale)).cuda()
    z_in, z_out = normal("z_in", (B, c, h, w)), normal("z_out", (B, T, c, h, w))
    g_pred, v0 = normal("g_pred", (B, T, c, h, w), 1.0), normal("v", (B, K, c, h, w), 1.0)
    obs, z_bg = normal("obs", (B, len(OBS_STEPS), c, h, w)), normal("z_bg", (B, c, h, w))
    prm = torch.from_numpy(filler.uniform01("param", B, tr.INPUT_SEED).astype(np.float32)).cuda() if cond else None

    def forward():
        return {"z_pred": eng.train_forward(params, z_in, T, param=prm)[0]}

    def backward():
        z_pred, ws = eng.train_forward(params, z_in, T, param=prm)
        res = eng.train_backward(params, z_in, z_pred, g_pred, ws, need_z_grad=True, need_param_grad=cond)
        out = {"grad/" + k: t for k, t in res[0].items()}
        out["grad_z_in"] = res[1]
        if cond:
            out["grad_param"] = res[2]
        out["state_only/grad_z_in"] = eng.train_backward(params, z_in, z_pred, g_pred, ws, need_z_grad=True, state_only=True)[1]
        return out

    def tangent():
        ws = torch.empty(eng.train_tangent_workspace_bytes(B, h, w, T, K), dtype=torch.uint8, device="cuda")
        eng.train_forward(params, z_in, T, param=prm, workspace=ws)
        v = v0.clone()
        return {"v": v, "jv_out": eng.train_tangent(params, v, T, ws, t0=T0, nsteps=NSTEPS, keep=True)}

    def step_clip():
        own = {k: p.clone() for k, p in params.items()}
        grads, m, s = ({k: torch.zeros_like(p) for k, p in own.items()} for _ in range(3))
        loss, norm = eng.train_step_clip(own, z_in, z_out, grads, m, s, engine.update_spec(1e-3, step=1, max_norm=MAX_NORM), param=prm)
        assert float(norm) > MAX_NORM, "max_norm %g does not clip a norm of %g" % (MAX_NORM, float(norm))
        out = {"loss": loss, "norm": norm}
        for tag, d in (("param", own), ("exp_avg", m), ("exp_avg_sq", s)):
            out.update({"%s/%s" % (tag, k): t for k, t in d.items()})
        return out

    def fit():
        z0, p = z_in.clone(), prm.clone() if cond else None
        st = [torch.zeros_like(z0) for _ in range(3)]
        pt = [torch.zeros_like(p) for _ in range(3)] if cond else [None] * 3
        spec = engine.fit_spec(OBS_STEPS, None, BACKGROUND, state=engine.update_spec(2e-3, step=1),
                               param=engine.update_spec(2e-3, step=1) if cond else None)
        loss, per = eng.fit_step(params, z0, obs, spec, param=p, z_background=z_bg, g_z=st[0], exp_avg_z=st[1], exp_avg_sq_z=st[2],
                                 g_p=pt[0], exp_avg_p=pt[1], exp_avg_sq_p=pt[2])
        out = {"z0": z0, "loss": loss, "per": per}
        if cond:
            out["param"] = p
        return out
    return eng, (("train_forward", forward), ("train_backward", backward), ("train_tangent", tangent),
                 ("train_step_clip", step_clip), ("fit_step", fit))


def bits():
    import train_reference as tr
    rec = {}
    for case in CASES:
        print("case", tr.case_id(case), file=sys.stderr, flush=True)
        eng, calls = case_calls(case)
        for form in FORMS:
            eng.set_option("train_wgrad", form)
            for name, call in calls:
                key = "%s/wgrad%d/%s" % (tr.case_id(case), form, name)
                rec[key], rec[key + "/not repeatable"] = twice(call)
                bad = [k for k in rec[key + "/not repeatable"] if k in MUST_REPEAT]
                assert not bad, "%s: %s did not repeat: choose another case" % (key, bad)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", action="store_true", help="the workspace size queries (host only) instead of the bits")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    text = rollout_bits.dumps(sizes() if a.sizes else bits())
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()

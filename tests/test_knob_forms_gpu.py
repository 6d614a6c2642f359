"""GPU: the form a launch reports is the form the launcher runs, under the switches that change it.  Three fresh child
processes (the switches are read once per process: csrc/lns_knobs.h) -- default, LNS_FA_SANDWICH_BF16X3=1, LNS_ATTN_FP32=1 --
each run a B = 2, T = 2 rollout of the ns2d_mini fixture with timing on and "fa_fused" 0.  ns2d_mini is the smallest fixture whose
plan holds both a plain FABlock sandwich op and an attention op (tools/rollout_bits.py "classes/ns2d_mini": fa_sandwich and
attention; ns2d_mini_sa has no FABlock).  Its planes are one 32 x 32 tile and both producers record max |.| per sample, so the
rules (fa_sandwich_form, attn_is_f16; tests/test_knobs_cpu.py derives them) give: f16x2 sandwich and f16x2 attention by default,
the bf16x3 sandwich under LNS_FA_SANDWICH_BF16X3, fp32 MFMA attention under LNS_ATTN_FP32.  The decoded steps meet the tolerance
tests/test_gpu_parity.py applies to the fixture's golden in every arm.

Run as a program, this file is the child: it prints one JSON line."""
import json
import os
import subprocess
import sys

import pytest

CASE, T = "ns2d_mini", 2
ARMS = {
    "default": ({}, "f16x2 FABlock sandwich", "f16x2 attention"),
    "sandwich_bf16x3": ({"LNS_FA_SANDWICH_BF16X3": "1"}, "bf16x3 FABlock sandwich", "f16x2 attention"),
    "attn_fp32": ({"LNS_ATTN_FP32": "1"}, "f16x2 FABlock sandwich", "fp32 MFMA attention"),
}


def child():
    import numpy as np  # noqa: F401
    import torch
    from helpers import load_golden, rel_l2, case_args, case_inputs, synthetic_state_dict
    from lns_amd import dropin
    meta, g = load_golden(CASE)
    args = case_args(meta)
    model = dropin.build_dynamics(args)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_state_dict(shapes, meta["weight_seed"]).items()}, strict=True)
    model = model.cuda()
    x, _ = case_inputs(meta, args)
    xd = torch.from_numpy(x).cuda()
    eng = model._engine(xd)
    eng.set_option("fa_fused", 0)
    eng.timing_enable(True)
    dec = eng.rollout(xd, T)
    torch.cuda.synchronize()
    timing = eng.timing()
    eng.timing_enable(False)
    dec = dec.cpu().numpy()
    sub = meta["sub"]
    errs = [rel_l2(dec[:, s - 1][..., ::sub, ::sub], g["dec"][:, i]) for i, s in enumerate(meta["steps"]) if s <= T]
    print(json.dumps({"forms": {k: v["launches"] for k, v in timing.items() if "/" in k}, "errs": [float(e) for e in errs],
                      "shape": list(dec.shape)}))


@pytest.mark.gpu
@pytest.mark.parametrize("arm", list(ARMS))
def test_reported_form_is_the_launched_form(arm):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from test_gpu_parity import ROLLOUT_TOL
    env_add, sandwich, attention = ARMS[arm]
    env = {k: v for k, v in os.environ.items() if not k.startswith("LNS_") or k == "LNS_HIP_LIB"}
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120,
                       env=dict(env, **env_add))
    assert r.returncode == 0, r.stdout + r.stderr
    rec = json.loads(r.stdout.splitlines()[-1])
    print(arm, rec)
    forms = rec["forms"]
    assert {k.split("/", 1)[1] for k in forms if k.startswith("fa_sandwich/")} == {sandwich}
    assert {k.split("/", 1)[1] for k in forms if k.startswith("attention/")} == {attention}
    assert rec["shape"][:2] == [2, T] and len(rec["errs"]) == 2
    assert all(e < ROLLOUT_TOL for e in rec["errs"]), rec["errs"]


if __name__ == "__main__":
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (_root, os.path.join(_root, "oracle"), os.path.dirname(os.path.abspath(__file__))):
        if _p not in sys.path:
            sys.path.insert(0, _p)
    child()

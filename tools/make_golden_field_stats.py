#!/usr/bin/env python3
"""Golden vectors of the field statistics (include/lns.h "field statistics"): the datasets' denormalize() followed by the
reference's own pointwise_correlation and by GradientDomainLoss.spatial_fd + relative_lp_loss, computed by the REAL
reference in float64 (imported on CPU through oracle/ref_shim.py; runs only in the build container).  The dataset classes
are not constructed (their data files do not exist here): denormalize() only reads `self.stats` / `self.normstat`, so it
is called on a bare namespace carrying those.

Committed: tests/golden/field_stats.npz = seed and, for the NS2d (scalar statistics), SW (per-channel statistics) and
two-phase (wall zeroing + VOF clamp) datasets, cos / grad_y / grad_x [B, T, C] in float64.  The inputs are regenerated from
the seed by tests/field_stats_reference.golden_inputs (data only; nothing of the reference's text is stored).

    python tools/make_golden_field_stats.py
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import ref_shim  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
import field_stats_reference as fr  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "field_stats.npz")


def main():
    ref_shim.load_reference()
    tu = importlib.import_module("training_utils")
    ns_ds = importlib.import_module("dataset.ns2d_fno_stage2_simpleae")
    sw_ds = importlib.import_module("dataset.Stage2_SW")
    tp_ds = importlib.import_module("dataset.twophase_flow_stage2")
    dt = torch.float64
    gdl = tu.GradientDomainLoss(1.0, 1.0)
    out = {"seed": np.int64(fr.GOLDEN_SEED)}
    for name in fr.GOLDEN:
        yh, y = fr.golden_inputs(name)
        a, g = torch.from_numpy(yh).to(dt), torch.from_numpy(y).to(dt)
        if name == "ns2d":
            st = fr.GOLDEN[name]["norm"]
            self = types.SimpleNamespace(stats={"mean": torch.tensor(st["mean"], dtype=dt), "std": torch.tensor(st["std"], dtype=dt)})
            den = lambda v: ns_ds.NS2DData.denormalize(self, v)
        elif name == "sw":
            st = fr.GOLDEN[name]["norm"]
            ns = {k: {"mean": torch.tensor(m, dtype=dt), "std": torch.tensor(s, dtype=dt)}
                  for k, m, s in zip(("u", "v", "pres"), st["mean"], st["std"])}
            self = types.SimpleNamespace(normstat=ns)
            den = lambda v: sw_ds.SW2DData.denormalize(self, v.clone())
        else:
            keys = ("vel_mean", "vel_std", "prs_mean", "prs_std")
            self = types.SimpleNamespace(stats={k: torch.tensor(v, dtype=dt) for k, v in zip(keys, fr.GOLDEN[name]["stats"])})
            den = lambda v: tp_ds.ConditionalTankSloshingData.denormalize(self, v)
        ad, gd = den(a), den(g)
        out[name + "_cos"] = tu.pointwise_correlation(ad, gd, reduce_dim=(3, 4)).numpy()
        (py, px), (qy, qx) = gdl.spatial_fd(ad), gdl.spatial_fd(gd)
        out[name + "_grad_y"] = tu.relative_lp_loss(py, qy, reduce_dim=(-1, -2), reduce_all=False).numpy()
        out[name + "_grad_x"] = tu.relative_lp_loss(px, qx, reduce_dim=(-1, -2), reduce_all=False).numpy()
        for k in ("cos", "grad_y", "grad_x"):
            v = out["%s_%s" % (name, k)]
            assert v.dtype == np.float64 and v.shape == tuple(fr.GOLDEN[name]["shape"][:3]), (name, k, v.shape, v.dtype)
        print(name, "cos[0,0]", out[name + "_cos"][0, 0], "grad_y[0,0]", out[name + "_grad_y"][0, 0])
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()

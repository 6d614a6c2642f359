"""Does localisation help?  The twin experiment of tests/test_etkf_cpu.py (etkf_reference.TWIN: ns2d_mini, B = 2, M = 8, every 4th
pixel of channel 0 observed at steps 0 and 2 with rinv = 1e4, one analysis per observed step) through the float64 CPU oracle and
the numpy statements, for the numpy noise seeds 1 .. 30, with the global filter (tests/etkf_reference.py) and with the localised
one (tests/letkf_reference.py, the independent statement) at the radii 0.5, 1, 2 and 1e9 latent pixels, side by side.  Per filter
and seed, at the last observed step: the weighted misfit of the analysis mean over the forecast mean's at the OBSERVED values (what
the filter minimises), and the same ratio of the plain squared misfit at the HELD-OUT values (every unobserved value of every
channel: what the filter was not shown).  A record, not a gate: the weights are synthetic and the decoder holds attention, so
nothing guarantees that a pixel's latent acts on its own patch alone.

    python tools/letkf_twin.py [--out profiles/letkf_twin.json] [--seeds 30]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

import etkf_reference as er  # noqa: E402
import letkf_reference as lr  # noqa: E402

RADII = (0.5, 1.0, 2.0, 1e9)


def held_out(frames, y, r):
    """sum over the values with r = 0 of (y - mean over the members)^2 per sample: frames [B, M, C, H, W], y [B, C, H, W]"""
    d = np.asarray(y, dtype=np.float64) - np.asarray(frames, dtype=np.float64).mean(1)
    return (d * d * (np.asarray(r) == 0)).sum((1, 2, 3))


def main():
    import lns_oracle
    from helpers import case_args, load_golden, manifest, synthetic_state_dict
    from lns_amd import filler
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "letkf_twin.json"))
    ap.add_argument("--seeds", type=int, default=30)
    a = ap.parse_args()
    t = er.TWIN
    meta, _ = load_golden(t["preset"])
    args = case_args(meta)
    sd = synthetic_state_dict({k: tuple(v) for k, v in manifest()[t["preset"]].items()}, meta["weight_seed"])
    orc = lns_oracle.OracleDynamics(args, sd)
    B, M = t["B"], t["M"]
    tail = (args.in_channels, args.Ly, args.Lx)
    x0 = filler.normal("x", (B,) + tail, t["x_seed"])
    z0 = orc.x_to_z(x0)
    grid = tuple(z0.shape[2:])
    bc = (lr.PERIODIC, lr.PERIODIC)                   # ns2d: the autoencoder pads both axes circularly

    def roll(z, steps):
        for _ in range(steps):
            z = orc.prop.forward(z)
        return z

    def decode(z):
        return orc.z_to_x(z).reshape((B, M) + tail)
    r = er.twin_rinv(*tail, t["rinv"])
    truth, zt, start = [], z0, 0
    for step in t["obs_steps"]:                       # the truth's frames at the observed steps, once
        zt = roll(zt, step + 1 - start)
        truth.append(orc.z_to_x(zt))
        start = step + 1
    filters = [("etkf", None)] + [("letkf_r%g" % rad, rad) for rad in RADII]
    rows = {name: dict(observed=[], held_out=[]) for name, _ in filters}
    for seed in range(1, a.seeds + 1):
        rng = np.random.default_rng(seed)
        zs = (z0[:, None] + t["noise_level"] * rng.standard_normal((B, M) + z0.shape[1:])).astype(np.float32)
        for name, rad in filters:
            z, start = zs.reshape((B * M,) + z0.shape[1:]), 0
            for y, step in zip(truth, t["obs_steps"]):
                z = roll(z, step + 1 - start)
                frames = decode(z)
                zz = z.reshape((B, M) + z0.shape[1:])
                if rad is None:
                    an = er.analysis(frames[None], y[:, None], r, zz.reshape(B, M, -1), 1.0)["z"]
                else:
                    an = lr.local_analysis(frames[None], y[:, None], r, zz, 1.0, grid, rad, bc)["z"]
                fc_obs, fc_held = er.misfit(frames, y, r), held_out(frames, y, r)
                z = an.astype(np.float32).reshape(z.shape)
                start = step + 1
            after = decode(z)
            rows[name]["observed"].append((er.misfit(after, y, r) / fc_obs).tolist())
            rows[name]["held_out"].append((held_out(after, y, r) / fc_held).tolist())
        print("seed %d:" % seed, {k: [round(float(np.mean(v["observed"][-1])), 3), round(float(np.mean(v["held_out"][-1])), 3)] for k, v in rows.items()},
              flush=True)

    def summary(v):
        flat = [x for row in v for x in row]
        return dict(min=round(min(flat), 4), median=round(statistics.median(flat), 4), max=round(max(flat), 4),
                    above_1=sum(x > 1.0 for x in flat), n=len(flat))
    rec = dict(tool="letkf_twin", settings=dict(t, noise_seeds=[1, a.seeds], latent_grid=list(grid), radii=list(RADII), boundary="periodic"),
               what="analysis / forecast at the last observed step, per sample (B = 2) and numpy noise seed: `observed` the weighted "
                    "misfit of the ensemble mean at the observed values, `held_out` the squared misfit at the unobserved values",
               summary={k: dict(observed=summary(v["observed"]), held_out=summary(v["held_out"])) for k, v in rows.items()},
               per_seed=rows)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec["summary"], indent=1))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What do the rollout entry points enqueue?  One JSON object: "case/entry/options" -> {output tensor: first 16 hex digits of the
sha256 of its bytes} for every rollout entry point of `Engine` (rollout, rollout with to_x=False, rollout with keep_steps,
rollout_latent, rollout_latent with keep_steps, rollout_eval, rollout_latent_eval in one chunk and in two, 4 + 3,
rollout_latent_ensemble with M = 3 members, rollout_latent_ensemble_eval, rollout_latent_ensemble_quantiles (three quantiles,
one threshold, mean / var / z_last as well), rollout_latent_ensemble_exceed (the same threshold against y; mean / var / z_last
as well) and rollout_latent_ensemble_analysis (every 4th pixel of channel 0 of y observed at the kept steps, rho = 1.1; z, X, wbar,
lam, stat, status, mean / var / z_last) and rollout_latent_ensemble_analysis_local (the same observations, radius 2 latent pixels,
return_X; every tensor it returns) on the same members where the library has them, and
the six newer scored calls -- rollout_eval_spectrum / _stats / _maps from x and their rollout_latent_ forms in two chunks, 4 + 3:
spectra at steps [0, 3, 6], statistics at [1, 2, 6] with an 8-bin histogram, maps from step 1 every 2, the _maps forms with all
three selections together; every tensor they return is hashed, the chunks' per-step tensors concatenated) under
decode_group {default, 1, 2, automatic} x decode_streams {1, 2} x overlap {0, 1}, at B = 2, T = 7 (decode_group = 2: a ragged last
group), keep_steps = [1, 4, 6], on the shapes of the ns2d_mini, twophase_cond and sw_half_periodic fixtures with inputs
from `filler`; plus "launches/<call>" -> {kernel class: launches} of one rollout, one rollout(keep_steps=...), one
rollout_eval and one rollout_eval_maps (all selections) of ns2d_mini under timing_enable(True).  An entry whose hashes are the
same under all 16 settings is written once, as "case/entry/all 16 settings"; one whose hashes differ keeps a key per setting.
Then, so that every kind of launch a plan can hold is reached, with the library's default options only: the ns2d_mini variants with self-attention, an attention encoder, Fourier blocks and two
residual blocks per level and the unconditional two-phase model (EXTRA), and ns2d_64 (the smallest preset whose FABlock fits
the fused kernel: 32 x 32 planes, 128 channels) under fa_fused 0 (plain sandwich), fa_fused 2 (input split + fused kernel) and
fa_fused 0 with fa_chunk_mb 1 (the in_proj -> sandwich -> to_out chain re-issued per sample); "classes/<case>[/<options>]" ->
{kernel class or class/form: launches} of one rollout of each case.  The tool fails if a kernel class of the library is
launched by none of them.  Beside the rollouts, the two other sites that build conv launches: "op_conv/<idx>" -> the output of
every op-level conv case of the kernel tests (tests/gpu_checks.py CONV_CASES) and "train/<case>" -> loss and parameter gradients
of one training step (train_wgrad 0) of ns2d_mini and twophase_cond at B = 2, T = 3, the tensors whose hashes repeat when the step
runs twice.  Two builds that enqueue the same work print the same object.

    python tools/rollout_bits.py [--out FILE]
"""
import argparse
import hashlib
import itertools
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from lns_amd import config, dropin, filler  # noqa: E402

CASES = ("ns2d_mini", "twophase_cond", "sw_half_periodic")
EXTRA = ("ns2d_mini_sa", "ns2d_mini_attn_enc", "ns2d_mini_attn_enc_sa", "ns2d_mini_fourier", "ns2d_mini_res2", "twophase")
FA_CASE = "ns2d_64"
FA_OPTIONS = (dict(fa_fused=0, fa_chunk_mb=0), dict(fa_fused=2, fa_chunk_mb=0), dict(fa_fused=0, fa_chunk_mb=1))
B, T = 2, 7
TRAIN_CASES, TRAIN_T = ("ns2d_mini", "twophase_cond"), 3
KEEP = [1, 4, 6]
CHUNKS = ((0, 4, [1]), (4, 3, [0, 2]))              # (t0, steps, keep_steps of the chunk): KEEP again
NORM = dict(mean=0.37, std=1.9)
MEMBERS, NOISE = 3, 0.05                            # rollout_latent_ensemble: z0 + NOISE * filler.normal per member
QUANTILES, THRESHOLDS = (0.05, 0.5, 0.95), (0.5,)      # rollout_latent_ensemble_quantiles, rollout_latent_ensemble_exceed
LOC_RADIUS = 2.0                                    # rollout_latent_ensemble_analysis_local
SPECTRUM_STEPS, STATS_STEPS, HIST, MAP_STEPS = [0, 3, 6], [1, 2, 6], (8, -4.0, 4.0), (1, 2)
DECODE_GROUPS = (None, 1, 2, 0)                     # None: never set (it comes first); 0: automatic, here one group of all T steps


def sha(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()[:16]     # 64 bits: the first 16 digits of earlier records


def merge_settings(rec):
    """The keys "case/entry/dg*_ds*_ov*" of one entry -> one key "case/entry/all N settings" when their N values are equal."""
    groups = {}
    for k in rec:
        m = re.fullmatch(r"(.*)/dg\w+_ds\d_ov\d", k)
        if m:
            groups.setdefault(m.group(1), []).append(k)
    for prefix, keys in groups.items():
        if all(rec[k] == rec[keys[0]] for k in keys):
            v = rec[keys[0]]
            for k in keys:
                del rec[k]
            rec["%s/all %d settings" % (prefix, len(keys))] = v
    return rec


def dumps(rec):
    """One key per line (a record has some 200 keys of up to nine hashes): two records compare line by line."""
    return "{\n" + ",\n".join(" %s: %s" % (json.dumps(k), json.dumps(rec[k], sort_keys=True)) for k in sorted(rec)) + "\n}"


def setup(name):
    print("case", name, file=sys.stderr, flush=True)
    d = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    meta = json.loads(bytes(d["meta"]).decode())
    args = config.preset(meta["preset"], **meta["overrides"])
    model = dropin.build_dynamics(args)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(v) for k, v in filler.synthetic_state_dict(shapes, meta["weight_seed"]).items()})
    model = model.to("cuda:0")
    seed = meta["input_seed"]
    x = torch.from_numpy(filler.normal("x", (B, args.in_channels, args.Ly, args.Lx), seed)).cuda()
    y = torch.from_numpy(filler.normal("y", (B, T, args.in_channels, args.Ly, args.Lx), seed)).cuda()
    p = torch.from_numpy(filler.uniform01("param", B, seed).astype(np.float32)).cuda() if args.family == "twophase_cond" else None
    return model._engine(x), x, y, p


def chunk_steps(steps, t0, n):
    """The steps of the horizon that fall into the chunk t0 .. t0 + n - 1, relative to it."""
    return [s - t0 for s in steps if t0 <= s < t0 + n]


def scored(res, z_last=None):
    """Every tensor of an Eval* result (a namedtuple; the step lists and rules among its fields are not tensors)."""
    d = {k: v for k, v in res._asdict().items() if isinstance(v, torch.Tensor)}
    if z_last is not None:
        d["z_last"] = z_last
    return d


def scored_chunks(call, z0, y, p, **sel):
    """One horizon in CHUNKS through a rollout_latent_eval_* call: frame / seq / maps are passed along, the per-step tensors
    of the chunks concatenated; **sel: the selections as steps of the horizon."""
    z, carry, parts = z0, {}, {}
    for t0, steps, keep in CHUNKS:
        rel = {k: chunk_steps(v, t0, steps) for k, v in sel.items() if k.endswith("_steps") and k != "map_steps"}
        res = call(z, y, steps=steps, t0=t0, param=p, keep_steps=keep, **dict(sel, **rel), **carry, **NORM)
        z = res.z_last
        carry = {k: getattr(res, k) for k in ("frame", "seq", "maps") if hasattr(res, k)}
        for k in ("frames", "spectra", "stats", "hist"):
            if getattr(res, k, None) is not None:
                parts.setdefault(k, []).append(getattr(res, k))
    return dict(carry, z_last=z, **{k: torch.cat(v, 1) for k, v in parts.items()})


def entries(eng, x, y, p):
    z0 = eng.encode(x, p) if eng.cfg.cond_encoder else eng.encode(x)
    out, lat = eng.rollout(x, T, param=p, return_latents=True)
    yield "rollout", dict(out=out, latents=lat)
    yield "rollout_latents_only", dict(out=eng.rollout(x, T, param=p, to_x=False))
    out, lat = eng.rollout(x, T, param=p, keep_steps=KEEP, return_latents=True)
    yield "rollout_keep", dict(out=out, latents=lat)
    out, z = eng.rollout_latent(z0, T, param=p)
    yield "rollout_latent", dict(out=out, z_last=z)
    out, z = eng.rollout_latent(z0, T, param=p, keep_steps=KEEP)
    yield "rollout_latent_keep", dict(out=out, z_last=z)
    frame, seq, frames = eng.rollout_eval(x, y, param=p, keep_steps=KEEP, **NORM)
    yield "rollout_eval", dict(frame=frame, seq=seq, frames=frames)
    frame, seq, frames, z = eng.rollout_latent_eval(z0, y, param=p, keep_steps=KEEP, **NORM)
    yield "rollout_latent_eval", dict(frame=frame, seq=seq, frames=frames, z_last=z)
    z, frame, seq, kept = z0, None, None, []
    for t0, steps, keep in CHUNKS:
        frame, seq, frames, z = eng.rollout_latent_eval(z, y, steps=steps, t0=t0, param=p, keep_steps=keep, frame=frame, seq=seq, **NORM)
        kept.append(frames)
    yield "rollout_latent_eval_4+3", dict(frame=frame, seq=seq, frames=torch.cat(kept, 1), z_last=z)
    if eng._L.lns_build_has(b"rollout_ensemble") == 1:           # (absent from a build that predates the entry point)
        noise = torch.from_numpy(filler.normal("ens", (B, MEMBERS) + tuple(z0.shape[1:]), 3)).cuda()
        ze = (z0[:, None] + NOISE * noise).contiguous()
        mean, var, z = eng.rollout_latent_ensemble(ze, T, param=p, keep_steps=KEEP, return_last=True)
        yield "rollout_latent_ensemble", dict(mean=mean, var=var, z_last=z)
        if eng._L.lns_build_has(b"ensemble_score") == 1:
            s = eng.rollout_latent_ensemble_eval(ze, y, T, param=p, keep_steps=KEEP, return_mean=True, return_var=True,
                                                 return_last=True, **NORM)
            yield "rollout_latent_ensemble_eval", dict(rel_l2=s.rel_l2, rmse=s.rmse, spread=s.spread, crps=s.crps, seq=s.seq,
                                                       rank=s.rank, mean=s.mean, var=s.var, z_last=s.z_last)
        if eng._L.lns_build_has(b"ensemble_quantiles") == 1:
            q = eng.rollout_latent_ensemble_quantiles(ze, T, QUANTILES, THRESHOLDS, param=p, keep_steps=KEEP, return_mean=True,
                                                      return_var=True, return_last=True, **NORM)
            yield "rollout_latent_ensemble_quantiles", dict(quantiles=q.quantiles, prob=q.prob, mean=q.mean, var=q.var, z_last=q.z_last)
        if eng._L.lns_build_has(b"ensemble_exceed") == 1:
            r = eng.rollout_latent_ensemble_exceed(ze, y, T, THRESHOLDS, param=p, keep_steps=KEEP, return_mean=True, return_var=True,
                                                   return_last=True, **NORM)
            yield "rollout_latent_ensemble_exceed", dict(table=r.table, mean=r.mean, var=r.var, z_last=r.z_last)
        if eng._L.lns_build_has(b"ensemble_etkf") == 1:
            rinv = torch.zeros(tuple(y.shape[2:]), device=y.device)
            rinv[0].view(-1)[::4] = 4.0                             # every 4th pixel of channel 0 observed
            r = eng.rollout_latent_ensemble_analysis(ze, y[:, KEEP].contiguous(), rinv, T, param=p, keep_steps=KEEP, rho=1.1,
                                                     return_mean=True, return_var=True, return_last=True, **NORM)
            yield "rollout_latent_ensemble_analysis", dict(z=r.z, X=r.X, wbar=r.wbar, lam=r.lam, stat=r.stat, status=r.status,
                                                           mean=r.mean, var=r.var, z_last=r.z_last)
            if eng._L.lns_build_has(b"ensemble_letkf") == 1:
                r = eng.rollout_latent_ensemble_analysis_local(ze, y[:, KEEP].contiguous(), rinv, T, LOC_RADIUS, param=p, keep_steps=KEEP,
                                                               rho=1.1, return_mean=True, return_var=True, return_last=True,
                                                               return_X=True, **NORM)
                yield "rollout_latent_ensemble_analysis_local", scored(r)
    for name, sel in (("spectrum", dict(spectrum_steps=SPECTRUM_STEPS)), ("stats", dict(stats_steps=STATS_STEPS, hist=HIST)),
                      ("maps", dict(map_steps=MAP_STEPS, stats_steps=STATS_STEPS, hist=HIST, spectrum_steps=SPECTRUM_STEPS))):
        if eng._L.lns_build_has(b"eval_" + name.encode()) == 1:
            yield "rollout_eval_" + name, scored(getattr(eng, "rollout_eval_" + name)(x, y, param=p, keep_steps=KEEP, **sel, **NORM))
            yield "rollout_latent_eval_%s_4+3" % name, scored_chunks(getattr(eng, "rollout_latent_eval_" + name), z0, y, p, **sel)


def launches(eng, x, y):
    calls = (("rollout", lambda: eng.rollout(x, T)), ("rollout_keep", lambda: eng.rollout(x, T, keep_steps=KEEP)),
             ("rollout_eval", lambda: eng.rollout_eval(x, y, keep_steps=KEEP, **NORM)),
             ("rollout_eval_maps", lambda: eng.rollout_eval_maps(x, y, keep_steps=KEEP, map_steps=MAP_STEPS, stats_steps=STATS_STEPS,
                                                                 hist=HIST, spectrum_steps=SPECTRUM_STEPS, **NORM)))
    rec = {}
    for name, fn in calls:
        eng.timing_enable(True)
        fn()
        torch.cuda.synchronize()
        rec["launches/" + name] = {k: v["launches"] for k, v in sorted(eng.timing().items())}
        eng.timing_enable(False)
    return rec


def classes(eng, x, p):
    """{kernel class or class/form: launches} of one rollout (timing mode: everything on the caller's stream)."""
    eng.timing_enable(True)
    eng.rollout(x, T, param=p)
    torch.cuda.synchronize()
    rec = {k: v["launches"] for k, v in sorted(eng.timing().items())}
    eng.timing_enable(False)
    return rec


def op_conv():
    """"op_conv/<idx>": the output of every op-level conv case of the kernel tests (tests/gpu_checks.py CONV_CASES, seeded by
    its index as tests/test_gpu_parity.py::test_conv_kernel seeds it) that the build compiles."""
    for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import gpu_checks
    from lns_amd import _lib
    experimental = _lib.lib().lns_build_has(b"experimental") == 1
    rec = {}
    for idx, case in enumerate(gpu_checks.CONV_CASES):
        if case.get("variant") in (15, 16, 18, 19, 20) and not experimental:      # forms of -DLNS_EXPERIMENTAL builds only
            continue
        rec["op_conv/%d" % idx] = {"y": sha(torch.from_numpy(np.ascontiguousarray(gpu_checks.conv_case(seed=idx, ret_y=True, **case)[2])))}
    return rec


def train(name):
    """"train/<case>": loss and every parameter gradient of one training step (train_wgrad 0, no update) at B = 2, T = 3.  The
    step runs twice on fresh gradients: a tensor whose hashes differ between the two (atomics) is not recorded but named."""
    from lns_amd import train as lns_train
    print("train", name, file=sys.stderr, flush=True)
    d = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    meta = json.loads(bytes(d["meta"]).decode())
    args = config.preset(meta["preset"], **meta["overrides"])
    model = dropin.build_dynamics(args)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(v) for k, v in filler.synthetic_state_dict(shapes, meta["weight_seed"]).items()})
    model = model.to("cuda:0")
    c, h, w = model._eng.latent_shape()
    z_in = torch.from_numpy(filler.normal("z_in", (B, 1, c, h, w), 5) * np.float32(0.5)).cuda()
    z_out = torch.from_numpy(filler.normal("z_out", (B, TRAIN_T, c, h, w), 5) * np.float32(0.5)).cuda()
    prm = (torch.from_numpy(filler.uniform01("param", B, 5).astype(np.float32)).cuda(),) if args.family == "twophase_cond" else ()
    tr = lns_train.Stage2Trainer(model, wgrad="tile")
    runs = []
    for _ in range(2):
        for p in model.propagator.parameters():
            p.grad = None
        loss = tr.step(z_in, z_out, *prm, update=False)
        torch.cuda.synchronize()
        runs.append(dict({"loss": sha(loss)}, **{"grad/" + k: sha(p.grad) for k, p in model.propagator.named_parameters()}))
    same = {k: v for k, v in runs[0].items() if runs[1][k] == v}
    return {"train/" + name: same, "train/%s/not repeatable" % name: sorted(set(runs[0]) - set(same))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rec = op_conv()
    for case in TRAIN_CASES:
        rec.update(train(case))
    for case in CASES:
        eng, x, y, p = setup(case)
        for dg, ds, ov in itertools.product(DECODE_GROUPS, (1, 2), (0, 1)):
            for k, v in (("decode_group", dg), ("decode_streams", ds), ("overlap", ov)):
                if v is not None:
                    eng.set_option(k, v)
            for name, tensors in entries(eng, x, y, p):
                torch.cuda.synchronize()
                rec["%s/%s/dg%s_ds%d_ov%d" % (case, name, "default" if dg is None else dg, ds, ov)] = {k: sha(t) for k, t in tensors.items()}
        if case == "ns2d_mini":
            for k, v in (("decode_group", 1), ("decode_streams", 3), ("overlap", 1)):      # the library's defaults
                eng.set_option(k, v)
            rec.update(launches(eng, x, y))
        rec["classes/" + case] = classes(eng, x, p)
    for case in EXTRA + (FA_CASE,):
        eng, x, y, p = setup(case)
        for opts in (FA_OPTIONS if case == FA_CASE else ({},)):
            for k, v in opts.items():
                eng.set_option(k, v)
            suffix = "".join("/%s%d" % kv for kv in sorted(opts.items()))
            for name, tensors in entries(eng, x, y, p):
                torch.cuda.synchronize()
                rec["%s/%s/default%s" % (case, name, suffix)] = {k: sha(t) for k, t in tensors.items()}
            rec["classes/" + case + suffix] = classes(eng, x, p)
    reached = {k for key, c in rec.items() if key.startswith("classes/") for k, n in c.items() if "/" not in k and n > 0}
    src = open(os.path.join(ROOT, "lns-latent-neural-pde-solver_amd", "csrc", "lns_engine.cpp")).read()
    every = set(re.findall(r'"([^"]+)"', re.search(r"kClsName\[CLS_COUNT\] = \{([^}]*)\}", src).group(1)))
    text = dumps(merge_settings(rec))
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)
    assert reached == every, "kernel classes no case launches: %s" % sorted(every - reached)


if __name__ == "__main__":
    main()

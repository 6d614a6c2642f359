#!/usr/bin/env python3
"""What do the op-level entry points (csrc/lns_ops.inc) compute?  One JSON object: "entry/case" -> {output tensor: sha256 of its
bytes}, one call of each entry point that holds device memory for the length of the call, on fixed seeded inputs at the smallest
shape its GPU test uses (the launch helpers and input sets are the tests' own where they have them):

  lns_op_conv2d              3x3 and 1x1, automatic variant, (2, 64, 16, 16)               tests/gpu_checks.py conv2d_gpu
  lns_op_conv_gn             the first grid case: partials + table; the first fold case    tests/test_conv_gn_stats_gpu.py
  lns_op_eval_attrib         (3, 2, 3, 17, 16), scalar spec                                tests/test_eval_attrib_gpu.py
  lns_op_latent_err          B 3, T 4, zper 33, zstride 36
  lns_op_groupnorm_stats     (2, 128, 105), one group, premul                              tests/test_gpu_parity.py
  lns_op_attention           B 2, 2 heads, D 32, n 16
  lns_op_fa_sandwich         B 2, 2 heads, C 32, 8 x 8
  lns_op_fa_fused            the grid's smallest case                                      tests/test_fa_fused_gpu.py
  lns_op_fa_reducer          scalar form (3, 7, 24, 48, 16); merged (3, 32, 64, 32) n 15 + 30    tests/test_fa_axis_gpu.py
  lns_op_fa_lrk              (2, 2, 64, 7); merged (3, 2, 64) n 7 + 15
  lns_op_ln_pe               (2, 5, 9) with and without the positional table               tests/test_ln_pe_apply_gpu.py
  lns_op_fourier_block       plain and conditional, the shapes of tests/golden/ops_fourier.npz
  lns_fourier_block_*        the same two blocks through the module objects: forward twice on the first sample (the second reuses
                             the prepared convolution), then once on the whole batch (scratch regrown, convolution prepared again)

Two builds that compute the same print the same object (LNS_HIP_LIB selects another build of the library).

    python tools/op_bits.py [--out FILE]
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from lns_amd import _lib, engine, filler  # noqa: E402


def sha(t):
    a = t.contiguous().cpu().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    return hashlib.sha256(a.tobytes()).hexdigest()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _hp(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def _ok(rc, what):
    torch.cuda.synchronize()
    assert rc == 0, (what, rc, _lib.lib().lns_create_error().decode())


def conv2d():
    import gpu_checks as gc
    r = np.random.default_rng(1)
    x = _dev(r.standard_normal((2, 64, 16, 16)))
    for k in (3, 1):
        w = (r.standard_normal((64, 64, k, k)) / np.sqrt(64 * k * k)).astype(np.float32)
        b = (0.1 * r.standard_normal(64)).astype(np.float32)
        yield "conv2d/k%d" % k, dict(y=gc.conv2d_gpu(x, w, b, k, pad=k // 2))


def conv_gn():
    import conv_gn_reference as cr
    import test_conv_gn_stats_gpu as t
    case = cr.GRID[0]
    _, out, _ = t._run(case)
    yield "conv_gn/" + case["name"], dict(y=out["y"], part=out["part"], ss=out["ss"], geom=np.array(list(out["geom"]), np.int32))
    name, cons = t.FOLD[0]
    _, out, _ = t._run(cr.BY_NAME[name], consumer=cons)
    yield "conv_gn/%s-v%d" % (name, cons[0]), dict(y=out["y"], part=out["part"], ss=out["ss"], y2=out["y2"])


def eval_attrib():
    L = _lib.lib()
    B, T, C, H, W = 3, 2, 3, 17, 16
    r = np.random.default_rng(2)
    y = r.standard_normal((B, T, C, H, W)).astype(np.float32)
    rec = (y + 0.2 * r.standard_normal(y.shape)).astype(np.float32)
    y_hat = (rec + 0.05 * r.standard_normal(y.shape) + 0.5 * (rec - y)).astype(np.float32)
    spec = engine.eval_spec(C, mean=0.37, std=1.9)
    outs = dict(prop_frame=_nan(B, T, C), prop_seq=_nan(B, C), cross_frame=_nan(B, T, C), cross_seq=_nan(B, C))
    d = [_dev(a) for a in (y_hat, rec, y)]
    _ok(L.lns_op_eval_attrib(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), B, T, C, H, W, ctypes.byref(spec),
                             *(outs[k].data_ptr() for k in ("prop_frame", "prop_seq", "cross_frame", "cross_seq")), _stream()), "eval_attrib")
    yield "eval_attrib/3x2x3x17x16", outs


def latent_err():
    L = _lib.lib()
    B, T, zper, zstride = 3, 4, 33, 36
    r = np.random.default_rng(3)
    zt = r.standard_normal((T, B, zper)).astype(np.float32)
    z = _dev(zt + 0.3 * r.standard_normal(zt.shape))
    staged = _nan(T, B, zstride)
    staged[..., :zper] = _dev(zt)
    outs = dict(frame=_nan(B, T), seq=_nan(B))
    _ok(L.lns_op_latent_err(z.data_ptr(), staged.data_ptr(), B, T, zper, zstride, 1e-8, outs["frame"].data_ptr(), outs["seq"].data_ptr(),
                            _stream()), "latent_err")
    yield "latent_err/B3T4z33", outs


def groupnorm_stats():
    L = _lib.lib()
    B, C, HW = 2, 128, 105
    r = np.random.default_rng(4)
    x = _dev(r.standard_normal((B, C, HW)) * 1.5 + 0.7)
    g, b = (1 + 0.1 * r.standard_normal(C)).astype(np.float32), (0.1 * r.standard_normal(C)).astype(np.float32)
    pm = _dev(1 + 0.3 * r.standard_normal((B, C)))
    ss = _nan(B, C, 2)
    _ok(L.lns_op_groupnorm_stats(x.data_ptr(), B, C, HW, 1, 1e-5, _hp(g), _hp(b), pm.data_ptr(), ss.data_ptr(), _stream()), "groupnorm_stats")
    yield "groupnorm_stats/2x128x105-premul", dict(ss=ss)


def attention():
    L = _lib.lib()
    B, heads, D, n = 2, 2, 32, 16
    qkv = _dev(np.random.default_rng(5).standard_normal((B, 3, heads, D, n)))
    o = _nan(B, heads, D, n)
    _ok(L.lns_op_attention(qkv.data_ptr(), B, heads, D, n, float(D) ** -0.5, o.data_ptr(), _stream()), "attention")
    yield "attention/B2h2D32n16", dict(o=o)


def fa_sandwich():
    L = _lib.lib()
    B, heads, C, H, W = 2, 2, 32, 8, 8
    r = np.random.default_rng(6)
    u = _dev(r.standard_normal((B, heads * C, H, W)))
    kx, ky = _dev(r.standard_normal((B, heads, H, H)) / np.sqrt(H)), _dev(r.standard_normal((B, heads, W, W)) / np.sqrt(W))
    o = _nan(B, heads * C, H, W)
    _ok(L.lns_op_fa_sandwich(u.data_ptr(), kx.data_ptr(), ky.data_ptr(), B, heads, C, H, W, 1e-5, 1, o.data_ptr(), _stream()), "fa_sandwich")
    yield "fa_sandwich/B2h2C32-8x8", dict(out=o)


def fa_fused():
    import fa_fused_reference as fr
    import test_fa_fused_gpu as t
    case = min(fr.GRID, key=lambda c: c["B"] * c["heads"] * c["dh"] * c["H"] * c["W"] * c["Cin"])
    out, amax = t.launch(case, fr.case_inputs(case))
    yield "fa_fused/" + case["name"], dict(out=out, amax=amax)


def fa_axis():
    import fa_axis_reference as fr
    import test_fa_axis_gpu as t
    import test_ln_pe_apply_gpu as tl
    (u, amax), = t.run_reducer([fr.reducer_set("zero_mean", 3, 7, 24, 48, 16)], 1)
    yield "fa_reducer/scalar-B3n7C24H48O16", dict(u=u, amax=amax)
    axes = [fr.reducer_set("zero_mean", 3, 15, 32, 64, 32, "x"), fr.reducer_set("zero_mean", 3, 30, 32, 64, 32, "y")]
    (ux, ax), (uy, ay) = t.run_reducer(axes, 0)
    yield "fa_reducer/merged-B3C32H64O32-n15x30", dict(ux=ux, amax_x=ax, uy=uy, amax_y=ay)
    k, = t.run_lrk([fr.lrk_set("std", 2, 2, 64, 7)], 1)
    yield "fa_lrk/B2h2D64n7", dict(k=k)
    kx, ky = t.run_lrk([fr.lrk_set("std", 3, 2, 64, 7, "x"), fr.lrk_set("std", 3, 2, 64, 15, "y")], 0)
    yield "fa_lrk/merged-B3h2D64-n7x15", dict(kx=kx, ky=ky)
    r = fr.lnpe_set(2, 5, 9)
    for with_pe in (False, True):
        h, bound = tl.run_ln_pe(r, with_pe)
        yield "ln_pe/2x5x9-pe%d" % with_pe, dict(h=h, bound=np.float32(bound))


def fourier():
    from lns_amd.modules.fourier_cond import CondFourierBasicBlock, FourierBasicBlock
    L = _lib.lib()
    d = np.load(os.path.join(ROOT, "tests", "golden", "ops_fourier.npz"))
    m = json.loads(bytes(d["meta"]).decode())
    B, C, H, W = m["B"], m["C"], m["H"], m["W"]
    x = _dev(filler.normal("xop", (B, C, H, W), m["input_seed"]))
    cond = _dev(filler.normal("cop", (B, C), m["input_seed"]))
    for name, cls in (("fourier", FourierBasicBlock), ("cond_fourier", CondFourierBasicBlock)):
        blk = cls(C, C, [m["m1"], m["m2"]])
        w = {}
        for ks in d[name + "_keys"]:
            k, shp = str(ks).split(":")
            w[k] = torch.from_numpy(filler.fill_tensor(k, tuple(int(v) for v in shp.split("x")), m["weight_seed"]))
        blk.load_state_dict(w, strict=True)
        conditional = name == "cond_fourier"
        host = [np.ascontiguousarray(t.detach().numpy(), dtype=np.float32) for t in blk._weights()] + [None] * (0 if conditional else 4)
        y = _nan(B, C, H, W)
        _ok(L.lns_op_fourier_block(x.data_ptr(), B, C, C, H, W, m["m1"], m["m2"], _hp(host[0]), _hp(host[1]), _hp(host[2]), _hp(host[3]),
                                   cond.data_ptr() if conditional else None, _hp(host[4]), _hp(host[5]), _hp(host[6]), _hp(host[7]),
                                   blk._act, int(blk.residual), y.data_ptr(), _stream()), name)
        yield "fourier_block/" + name, dict(y=y)
        run = (lambda xx, cc: blk(xx, cc)) if conditional else (lambda xx, cc: blk(xx))
        x1, c1 = x[:1].contiguous(), cond[:1].contiguous()
        yield "fourier_handle/" + name, dict(first=run(x1, c1), same_shape=run(x1, c1), larger=run(x, cond))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    rec = {}
    for group in (conv2d, conv_gn, eval_attrib, latent_err, groupnorm_stats, attention, fa_sandwich, fa_fused, fa_axis, fourier):
        for key, tensors in group():
            torch.cuda.synchronize()
            rec[key] = {k: sha(v) for k, v in tensors.items()}
    text = json.dumps(rec, indent=1, sort_keys=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()

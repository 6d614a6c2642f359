"""CPU: the batch-parallel weight gradient (option "train_wgrad", lns_op_conv_wgrad, include/lns.h) is declared and exported,
its option refuses unknown values, and the training workspaces are sized without a GPU: option 1 = option 0 plus the
documented partial-sum area, option 0 = what it was without the feature."""
import ctypes
import os
import re

import pytest

from helpers import ROOT

SYMBOLS = ("lns_op_conv_wgrad_scratch_bytes", "lns_op_conv_wgrad")
# the four recorded training shapes (tools/train_time.py) and a B = 1 case
SHAPES = [("ns2d_64", 32, 2), ("sw_half_periodic", 32, 5), ("twophase_cond", 32, 5), ("ns2d_128", 32, 2), ("ns2d_64", 1, 2)]


def _engine(preset="ns2d_mini"):
    from lns_amd import config, engine
    a = config.preset(preset)
    return a, engine.Engine(engine.make_config(a, ae_prefix="ae." if a.family == "twophase_cond" else "vq_ae.",
                                               prop_prefix="propagator."))


def test_wgrad_symbols_are_declared_and_exported():
    from lns_amd import _lib
    _lib.build()
    src = open(os.path.join(ROOT, "include", "lns.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(lns_[a-z0-9_]+)\s*\(", src))
    L = ctypes.CDLL(_lib.LIB_PATH)
    for s in SYMBOLS:
        assert s in declared, "not declared in include/lns.h: " + s
        assert hasattr(L, s), "missing export: " + s
        assert s in _lib.SYMBOLS
    assert re.search(r"#define\s+LNS_ABI_VERSION\s+2\b", src) and _lib.LNS_ABI_VERSION == 2
    assert _lib.lib().lns_build_has(b"train_wgrad_split") == 1


def test_train_wgrad_option_takes_0_and_1_only():
    from lns_amd import _lib
    from lns_amd._lib import LnsError
    _, e = _engine()
    L = _lib.lib()
    for bad in (2, -1):
        assert L.lns_set_option(e._h, b"train_wgrad", bad) == _lib.LNS_EINVAL
        with pytest.raises(LnsError):
            e.set_option("train_wgrad", bad)
    assert L.lns_set_option(e._h, b"train_wgrad", 1) == 0
    assert L.lns_set_option(e._h, b"train_wgrad", 0) == 0
    e.set_option("train_wgrad", 1)
    assert e.options["train_wgrad"] == 1


def _sizes(e, B, h, w, T):
    from lns_amd import _lib
    L = _lib.lib()
    a, b = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert L.lns_train_workspace_bytes(e._h, B, h, w, T, ctypes.byref(a)) == 0, L.lns_last_error(e._h)
    assert L.lns_train_step_workspace_bytes(e._h, B, h, w, T, ctypes.byref(b)) == 0, L.lns_last_error(e._h)
    assert e.train_step_workspace_bytes(B, h, w, T) == b.value
    return a.value, b.value


def _scratch(B, Cin, Cout, h, w, k, form=1):
    from lns_amd import _lib
    n = ctypes.c_size_t(123)
    assert _lib.lib().lns_op_conv_wgrad_scratch_bytes(B, Cin, Cout, h, w, k, form, ctypes.byref(n)) == 0
    return n.value


@pytest.mark.parametrize("preset,B,T", SHAPES)
def test_option_1_adds_exactly_the_partial_area(preset, B, T):
    """lns_train_workspace_bytes and lns_train_step_workspace_bytes under option 1 = their option-0 values + the largest
    S * Cout * Cin * k^2 floats (rounded to 64 floats) over the plan's five convolution geometries; 1 -> 0 restores the
    option-0 sizes; a fresh engine (option never touched) has the option-0 sizes."""
    args, e = _engine(preset)
    c, h, w = e.latent_shape()
    D = args.prop_n_embd
    base = _sizes(e, B, h, w, T)
    e.set_option("train_wgrad", 1)
    split = _sizes(e, B, h, w, T)
    geoms = [(c, D, 1), (D, c, 1), (D, D, 1), (D, D, 3)]
    area = max(_scratch(B, ci, co, h, w, k) for ci, co, k in geoms)
    assert area > 0 and area % 256 == 0
    # the op's size is S * Cout * Cin * k^2 floats for a whole number of slices S >= 1, at most one slice per (sample, chunk)
    for ci, co, k in geoms:
        per = co * ci * k * k * 4
        n = _scratch(B, ci, co, h, w, k)
        S = n // per                                    # (the rounding adds < 256 bytes < per)
        assert 1 <= S <= B * -(-h * w // 64) and (S * per + 255) // 256 * 256 == n, (ci, co, k, n, S)
        assert _scratch(B, ci, co, h, w, k, form=0) == 0
    assert split[0] == base[0] + area, (base, split, area)
    assert split[1] == base[1] + area, (base, split, area)
    e.set_option("train_wgrad", 0)
    assert _sizes(e, B, h, w, T) == base
    _, fresh = _engine(preset)
    assert _sizes(fresh, B, h, w, T) == base


def test_short_workspace_is_refused_under_option_1_before_any_device_work():
    """A workspace of the option-0 size is LNS_ENOMEM under option 1 (fake pointers, no GPU: nothing was enqueued), and the
    message names the needed size."""
    from lns_amd import _lib
    L = _lib.lib()
    _, e = _engine()
    c, h, w = e.latent_shape()
    B, T = 3, 2
    small = e.train_step_workspace_bytes(B, h, w, T)
    e.set_option("train_wgrad", 1)
    need = e.train_step_workspace_bytes(B, h, w, T)
    assert need > small
    arrs = []
    for _ in range(2):
        a = (ctypes.c_void_p * len(e.params))()
        for i, (k, _s, isb) in enumerate(e.params):
            if k.startswith("propagator.") and not isb:
                a[i] = 0x1000
        arrs.append(a)
    P = ctypes.c_void_p(0x1000)
    rc = L.lns_train_step(e._h, arrs[0], P, P, None, B, h, w, T, 1.0, arrs[1], None, None, None, P, P, small, None)
    assert rc == _lib.LNS_ENOMEM
    assert str(need) in L.lns_last_error(e._h).decode()


def test_op_refuses_bad_arguments_without_a_device():
    from lns_amd import _lib
    L = _lib.lib()
    P = ctypes.c_void_p(0x1000)

    def call(dy=P, x=P, B=2, Cin=16, Cout=16, H=8, W=8, k=3, dil=1, py=1, px=1, form=1, acc=0, dw=P, scratch=P, nbytes=1 << 40):
        return L.lns_op_conv_wgrad(dy, x, B, Cin, Cout, H, W, k, dil, py, px, form, acc, dw, scratch, nbytes, None)
    for kw in (dict(dy=None), dict(x=None), dict(dw=None), dict(B=0), dict(Cin=0), dict(H=0), dict(k=2), dict(k=5), dict(dil=0),
               dict(py=7), dict(px=-1), dict(form=2), dict(form=-1), dict(acc=2)):
        assert call(**kw) == _lib.LNS_EINVAL, kw
        assert "conv_wgrad" in L.lns_create_error().decode(), kw
    assert call(nbytes=16) == _lib.LNS_ENOMEM and "scratch" in L.lns_create_error().decode()
    assert call(scratch=None) == _lib.LNS_ENOMEM
    n = ctypes.c_size_t(0)
    assert L.lns_op_conv_wgrad_scratch_bytes(2, 16, 16, 8, 8, 3, 2, ctypes.byref(n)) == _lib.LNS_EINVAL
    assert L.lns_op_conv_wgrad_scratch_bytes(2, 16, 16, 8, 8, 3, 1, None) == _lib.LNS_EINVAL


def test_trainer_refuses_unknown_wgrad_names():
    from lns_amd import config, dropin, train
    from lns_amd._lib import LnsError
    m = dropin.build_dynamics(config.preset("ns2d_mini"))
    with pytest.raises(LnsError, match="wgrad"):
        train.Stage2Trainer(m, wgrad="fast")
    tr = train.Stage2Trainer(m, wgrad="split")
    assert m._owner._eng.options["train_wgrad"] == 1
    tr.set_wgrad("tile")
    assert m._owner._eng.options["train_wgrad"] == 0
    train.Stage2Trainer(m)                                       # None leaves the option alone
    assert m._owner._eng.options["train_wgrad"] == 0

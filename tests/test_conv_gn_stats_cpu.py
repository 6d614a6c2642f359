"""CPU: the grid of tests/conv_gn_reference.py would catch a subtly wrong statistics merge.  The producer's output is evaluated
in float64 and rounded to float32 (what the GPU test reads back from the device), the per-tile partials are taken in float64,
and four deliberate mistakes are applied to their merge: each must exceed 10 x the bound the GPU test holds the (scale, shift)
table to on at least one case, and the unmistaken float64 merge must stay below a tenth of it on every case."""
import functools

import numpy as np
import pytest

import conv_gn_reference as cr


def test_build_advertises_the_entry_point():
    """... and its argument checks need no device: they come before the first HIP call."""
    from lns_amd import _lib
    L = _lib.lib()
    assert L.lns_build_has(b"op_conv_gn") == 1
    assert L.lns_op_conv_gn(None, None) == _lib.LNS_EINVAL and L.lns_create_error().startswith(b"conv_gn: ")
    a = _lib.LnsConvGnArgs()
    assert L.lns_op_conv_gn(a, None) == _lib.LNS_EINVAL and b"null" in L.lns_create_error()


@functools.lru_cache(maxsize=None)
def _case_data(name):
    case = cr.BY_NAME[name]
    inp = cr.case_inputs(case)
    y = cr.producer64(case, inp)
    tiles = cr.tile_pixels(cr.expected_geom(case), case["H"], case["W"])
    return case, inp, y, cr.partials64(y, tiles)


def _worst(name, mistake):
    """max over samples of (error of the merged table against the float64 normalisation) / (the GPU test's bound)."""
    case, inp, y, (mean, m2, n) = _case_data(name)
    scale, shift = cr.merge64(mean, m2, n, case["groups"], cr.eps_of(case), inp["gamma"], inp["beta"], inp["premul"], mistake)
    return max([err / bound for _, err, _, bound in cr.table_errors(case, y, scale, shift, inp)] or [0.0])


def test_grid_covers_every_class():
    """Producer forms, planner modes, merge forms, kinds and epilogue features the grid has to hold."""
    rules = {c["name"]: cr.expected_rule(c) for c in cr.GRID}
    for prod, modes in (("c3", {0, 1, 2}), ("c3h", {0, 1}), ("up", {0}), ("c1", {0, 1, 2})):
        assert {rules[c["name"]][0] for c in cr.GRID if c["prod"] == prod} == modes, prod
    assert {c["kind"] for c in cr.GRID} == set(cr.KINDS) | {"mixed"}
    assert {c["feature"] for c in cr.GRID} == {None, "res", "badd_gelu", "oct"}
    fold = [c for c in cr.GRID if rules[c["name"]][1]]
    assert {(c["Cout"], c["groups"]) for c in fold} >= {(64, 32), (64, 1), (128, 32), (128, 1), (512, 1)}
    assert any(c["premul"] and c["groups"] == 1 for c in fold)
    assert any(c["premul"] and c["groups"] > 1 and not rules[c["name"]][1] for c in cr.GRID)
    assert not any(rules[c["name"]][1] for c in cr.GRID if c["Cout"] == 100 or c["prod"] == "up")
    assert any(rules[c["name"]][2] * c["Cout"] > 256 and c["groups"] == 1 for c in fold)       # second trip of the block-wide loop
    for c in cr.GRID:                                    # every tile holds pixels, and the tiles partition the plane
        px = np.concatenate(cr.tile_pixels(cr.expected_geom(c), c["H"], c["W"]))
        assert sorted(px) == list(range(c["H"] * c["W"])), c["name"]


@pytest.mark.parametrize("name", [c["name"] for c in cr.GRID])
def test_float64_merge_is_far_below_the_bound(name):
    w = _worst(name, None)
    assert w < 0.1, (name, w)


@pytest.mark.parametrize("mistake", cr.MISTAKES)
def test_mistake_is_caught(mistake):
    worst = {c["name"]: _worst(c["name"], mistake) for c in cr.GRID}
    top = max(worst, key=worst.get)
    print("%s: %d of %d cases beyond 10 x the bound; largest %.3g x at %s" % (mistake, sum(v > 10.0 for v in worst.values()),
                                                                                len(worst), worst[top], top))
    assert worst[top] > 10.0, (mistake, top, worst[top])

"""CPU: the workspace sizes of the training calls are what they were.

tests/golden/train_workspace_bytes.json records the five size queries (lns_train_workspace_bytes, lns_train_step_workspace_bytes,
lns_train_step_clip_workspace_bytes, lns_train_tangent_workspace_bytes, lns_fit_step_workspace_bytes) over four presets x three
(B, T) x both "train_wgrad" values x K in {1, 5} x n_obs in {1, 3}, written by `tools/train_bits.py --sizes` from the library
before the layout code (train_layout, the conv table, the tape view) was rewritten.  A workspace a caller sized with an earlier
build must stay the size a later build asks for, byte for byte."""
import json
import os
import sys

from helpers import ROOT


def test_workspace_sizes_are_the_recorded_ones():
    from lns_amd import _lib
    _lib.build()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import train_bits
    with open(os.path.join(ROOT, "tests", "golden", "train_workspace_bytes.json")) as f:
        want = json.load(f)
    got = train_bits.sizes()
    assert len(want) == len(train_bits.SIZE_PRESETS) * len(train_bits.SIZE_BT) * len(train_bits.FORMS) and all(len(r) == 7 for r in want.values())
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key] == want[key], (key, got[key], want[key])
    # the two forms size the workspace differently somewhere: the record does not hold one form twice
    assert any(want[k] != want[k.replace("wgrad0", "wgrad1")] for k in want if k.endswith("wgrad0"))

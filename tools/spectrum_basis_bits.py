"""The bits of the DFT / DFT energy spectra, as a record to compare two builds of the library by.

Hashes (sha256 of the float32 bytes) what lns_op_energy_spectrum returns on the inputs of tests/spectrum_reference.cases for a
list of planes -- with and without the truth -- and merges the record into a JSON file under `--key`.  Run it once with the
parent's library (LNS_HIP_LIB=<path> selects it) and once with this tree's; the two records must be equal key for key:

    LNS_HIP_LIB=/path/to/parent/liblns_hip.so python tools/spectrum_basis_bits.py --key parent
    python tools/spectrum_basis_bits.py --key branch --compare parent          # exits 1 if a hash differs
"""
import argparse
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from lns_amd import _lib, metrics  # noqa: E402
import spectrum_reference as sr  # noqa: E402

PLANES = ((1, 7), (2, 2), (3, 5), (16, 16), (29, 57), (32, 32), (33, 33), (24, 40), (61, 121), (121, 61), (96, 192), (192, 96), (128, 128))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--key", required=True)
    ap.add_argument("--compare", default=None, help="another key of the file: every hash must equal that record's")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectrum_basis_bits.json"))
    a = ap.parse_args()
    L = _lib.lib()
    rec = {}
    for H, W in PLANES:
        for name, y_hat, y, norm in sr.cases(H, W):
            yh, yt = torch.from_numpy(y_hat).cuda(), torch.from_numpy(y).cuda()
            for tag, truth in (("3 rows", yt), ("forecast only", None)):
                e = metrics.energy_spectrum(yh, truth, **norm)
                torch.cuda.synchronize()
                rec["%s, %s" % (name, tag)] = hashlib.sha256(e.cpu().numpy().tobytes()).hexdigest()
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            doc = json.load(f)
    doc[a.key] = dict(library=os.environ.get("LNS_HIP_LIB") and "LNS_HIP_LIB" or "this tree", spectrum_basis=int(L.lns_build_has(b"spectrum_basis")),
                      device=torch.cuda.get_device_name(0), hashes=rec)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%s: %d spectra hashed" % (a.key, len(rec)))
    if a.compare:
        other = doc[a.compare]["hashes"]
        diff = sorted(k for k in set(rec) | set(other) if rec.get(k) != other.get(k))
        print("%s against %s: %s" % (a.key, a.compare, "equal key for key" if not diff else "%d differ: %s" % (len(diff), diff[:5])))
        doc["equal"] = not diff
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")
        sys.exit(1 if diff else 0)


if __name__ == "__main__":
    main()

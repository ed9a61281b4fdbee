#!/usr/bin/env python3
"""tests/golden/dot_sites.npz: what the compiled reference (oracle/_ref) writes for the input families of tests/dot_sites_inputs.py --
payload bytes and the two lengths of every packet, per family; the generator fails if the reference does not encode a packet
(0 < n0 <= slot).  Run from the repository root after __graft_entry__.build()."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import dot_sites_inputs as B  # noqa: E402

out = {}
for name in B.FAMILIES + (B.WB,):
    bits, nb = B.reference(name)
    assert (nb[:, :, 0] > 0).all() and (nb[:, :, 0] <= B.SLOT).all(), name
    out[name + "/bits"], out[name + "/nbytes"] = bits, nb
    print("%-26s payload bytes %3d .. %3d" % (name, nb[:, :, 0].min(), nb[:, :, 0].max()))
np.savez_compressed(os.path.join(ROOT, "tests", "golden", "dot_sites.npz"), **out)

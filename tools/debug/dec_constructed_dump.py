#!/usr/bin/env python3
"""Writes the payloads of tests/golden/dec_constructed.npz / dec_constructed_wb.npz as flat files for tools/debug/dec_constructed_host.cpp (the
stand-alone sanitizer run of the decoder source): PREFIX_nb.bin, PREFIX_wb.bin.  Per stream int32 (flags of emu_dec_create, packets), per
packet int32 (nBytes0, nBytes1, lostflag, bytes handed over) and the bytes, mapped as the batched API maps a record (dec_stages_lib.map_record)."""
import os
import sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "tests")]
import dec_stages_lib as L

for rate, name in (("nb", "dec_constructed.npz"), ("wb", "dec_constructed_wb.npz")):
    z = np.load(os.path.join(ROOT, "tests", "golden", name))
    with open("%s_%s.bin" % (sys.argv[1], rate), "wb") as f:
        for k in range(int(z["n_streams"])):
            g = lambda n: z["s%02d_%s" % (k, n)]
            sr, total, md, joint, dtx, ms, P, cpk, reason = (int(v) for v in g("params"))
            f.write(np.array([md | joint << 1 | (8 if ms == 20 else 0), P], np.int32).tobytes())
            for p in range(P):
                off, a0, a1, lf = L.map_record(int(g("nbytes")[p, 0]), int(g("nbytes")[p, 1]), int(g("recv")[p]), 4 if (joint or ms == 20) else 8)
                n = 0 if lf == 1 else a0
                f.write(np.array([a0, a1, lf, n], np.int32).tobytes() + g("bits")[p, off:off + n].tobytes())

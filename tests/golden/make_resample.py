#!/usr/bin/env python3
"""Writes tests/golden/resample.npz: what the compiled fixed-point reference (oracle/_ref/libsolo_ref_fix.so, SKP_Silk_resampler_init /
SKP_Silk_resampler through ctypes) makes of the six input rows of tests/resample_lib.py.  Runs in the build container only.

For each of the eight pairs: the six rows' outputs for 4 packets of 40 ms, fed one packet per call, and the first 96 bytes of the
state (sIIR, sFIR, sDown2) after every packet; for 48 -> 16 and 16 -> 48 the same for packets of 20 ms.  The fixture holds no inputs.

In the 1.5x and 3x up paths the reference saves 24 bytes of an int16 buffer of which only the first 12 were written in the call (the
rest is whatever its stack held); the next call overwrites them before it reads them.  Those 12 bytes (sFIR[3..6)) are recorded as
zero, which is what the state holds after a reset.
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import resample_lib as L  # noqa: E402

LIB = os.path.join(ROOT, "oracle", "_ref", "libsolo_ref_fix.so")
STATE_BUF = 1024                                            # more than the reference's struct


class Ref:
    def __init__(self, lib, fs_in, fs_out):
        self.lib = lib
        self.S = (C.c_uint8 * STATE_BUF)()
        assert lib.SKP_Silk_resampler_init(self.S, fs_in, fs_out) == 0
        self.ratio = (fs_out, fs_in)
        self.dead = fs_out in (fs_in * 3, fs_in * 3 // 2) and fs_out > fs_in and fs_out != 2 * fs_in

    def run(self, x):
        x = np.ascontiguousarray(x, dtype=np.int16)
        n_out = x.size * self.ratio[0] // self.ratio[1]
        out = np.full(n_out + 64, 0x5A5A, dtype=np.int16)
        assert self.lib.SKP_Silk_resampler(self.S, out.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p), x.size) == 0
        assert np.all(out[n_out:] == 0x5A5A), "the reference wrote beyond the expected output"
        return out[:n_out].copy()

    def state(self):
        s = np.frombuffer(bytes(self.S)[:L.STATE_BYTES], dtype=np.uint8).copy()
        if self.dead:
            s[24 + 12: 24 + 24] = 0
        return s


def load():
    lib = C.CDLL(LIB)
    lib.SKP_Silk_resampler_init.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    lib.SKP_Silk_resampler.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
    return lib


def record(lib, fs_in, fs_out, ms, seed=L.SEED):
    x = L.inputs(fs_in, ms, seed)
    pcm, st = [], []
    for f in range(L.FAMILIES):
        r = Ref(lib, fs_in, fs_out)
        po, so = [], []
        for p in range(L.PACKETS):
            po.append(r.run(x[f, p]))
            so.append(r.state())
        pcm.append(np.stack(po))
        st.append(np.stack(so))
    return np.stack(pcm), np.stack(st)


def main():
    lib = load()
    out = {}
    for pairs, ms in ((L.PAIRS, 40), (L.PAIRS_20MS, 20)):
        for fs_in, fs_out in pairs:
            pcm, st = record(lib, fs_in, fs_out, ms)
            out["pcm_" + L.key(fs_in, fs_out, ms)] = pcm
            out["state_" + L.key(fs_in, fs_out, ms)] = st
    np.savez_compressed(L.FIXTURE, **out)
    print("wrote %s: %d arrays, %d bytes" % (L.FIXTURE, len(out), os.path.getsize(L.FIXTURE)))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Writes tests/golden/vad.npz: what the compiled fixed-point reference (oracle/_ref/libsolo_ref_fix.so, SKP_Silk_VAD_Init /
SKP_Silk_VAD_GetSA_Q8 through ctypes) makes of the rows of tests/vad_lib.py.  Runs in the build container only.

For frames of 320 and of 160 samples: the six rows' SA_Q8 and {SNR_dB_Q7, Tilt_Q15, Quality_Q15[4]} of every frame of 16 packets of 640
samples, and the 112 bytes of the state after every packet.  For frames of 320 the long row as well: SA_Q8 of all its 1040 frames and
the state after each of its last 32 packets.  The fixture holds no inputs.  Before anything is written the script asserts that the
rows reach the cases the tests rely on (see check()).
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vad_lib as L  # noqa: E402

LIB = os.path.join(ROOT, "oracle", "_ref", "libsolo_ref_fix.so")
STATE_BUF = 1024                                            # more than the reference's struct


class Ref:
    def __init__(self, lib):
        self.lib = lib
        self.S = (C.c_uint8 * STATE_BUF)()
        for i in range(L.REF_BYTES, STATE_BUF):
            self.S[i] = 0xA5
        assert lib.SKP_Silk_VAD_Init(self.S) == 0

    def frame(self, x):
        x = np.ascontiguousarray(x, dtype=np.int16)
        sa, snr, tilt = C.c_int(), C.c_int(), C.c_int()
        q = (C.c_int * 4)()
        assert self.lib.SKP_Silk_VAD_GetSA_Q8(self.S, C.byref(sa), C.byref(snr), q, C.byref(tilt), x.ctypes.data_as(C.c_void_p), x.size) == 0
        assert 0 <= sa.value <= 255
        return sa.value, [snr.value, tilt.value] + list(q)

    def packet(self, x, frame):
        out = [self.frame(x[f:f + frame]) for f in range(0, x.size, frame)]
        return np.array([o[0] for o in out], dtype=np.uint8), np.array([o[1] for o in out], dtype=np.int32)

    def state(self):
        b = bytes(self.S)
        assert all(v == 0xA5 for v in b[L.REF_BYTES:]), "the reference's state is larger than 112 bytes"
        return np.frombuffer(b[:L.REF_BYTES], dtype=np.uint8).copy()


def load():
    lib = C.CDLL(LIB)
    lib.SKP_Silk_VAD_Init.argtypes = [C.c_void_p]
    lib.SKP_Silk_VAD_GetSA_Q8.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    return lib


def record(lib, frame, seed=L.SEED):
    """-> sa uint8 [ROWS, PACKETS, F], detail int32 [ROWS, PACKETS, F, 6], state uint8 [ROWS, PACKETS, 112]"""
    x = L.inputs(seed)
    sa, det, st = [], [], []
    for r in range(L.ROWS):
        ref = Ref(lib)
        out = []
        for p in range(L.PACKETS):
            out.append(ref.packet(x[r, p], frame) + (ref.state(),))
        sa.append(np.stack([o[0] for o in out]))
        det.append(np.stack([o[1] for o in out]))
        st.append(np.stack([o[2] for o in out]))
    return np.stack(sa), np.stack(det), np.stack(st)


def record_long(lib, seed=L.SEED):
    """-> sa uint8 [LONG_PACKETS, 2], state uint8 [LONG_KEPT, 112], state uint8 [112] after the square wave"""
    x = L.long_input(seed)
    ref = Ref(lib)
    sa, st = [], []
    for p in range(L.LONG_PACKETS):
        sa.append(ref.packet(x[p], 320)[0])
        if p >= L.LONG_PACKETS - L.LONG_KEPT:
            st.append(ref.state())
        if p == L.LONG_SQUARE - 1:
            sq = ref.state()
    return np.stack(sa), np.stack(st), sq


def words(state):
    return state.view("<i4").reshape(state.shape[:-1] + (L.REF_BYTES // 4,))


def check(z):
    """the cases the tests rely on (tests/test_vad_model.py asserts the same on the committed file)"""
    for n in L.FRAMES:
        sa, st = z["sa_%d" % n].reshape(L.ROWS, -1), words(z["state_%d" % n])
        if n == 160:                                        # (32 frames of 320 cannot get there: tests/vad_lib.py; the long row does)
            assert np.all(st[2, -1, 15:19] == 0x00FFFFFF), ("row 2: the noise levels reach their ceiling", n, st[2, -1, 15:19])
        onset = int(np.argmax(sa[0] >= 200))
        assert sa[0].max() >= 200 and onset > 0 and sa[0, :onset].min() <= 8, ("row 0: silence, then speech", n, sa[0])
        assert sa[1, 0] >= 128 and sa[1, -1] <= 64, ("row 1: the tracker adapts to stationary noise", n, sa[1])
        assert np.all(sa[3] == 2) and list(st[3, -1, 15:19]) == [50, 25, 16, 12], ("row 3: silence", n, sa[3], st[3, -1, 15:19])
        assert np.any(sa[5, sa.shape[1] // 2:] <= 2), ("row 5: loud noise, then nothing", n, sa[5])
    assert np.all(words(z["state_long_square"])[15:19] == 0x00FFFFFF), ("the long row's square wave: every band at the ceiling", words(z["state_long_square"])[15:19])
    counter = words(z["state_long"])[:, 27]
    assert counter[0] < 1000 < counter[-1], ("the recorded states span the counter >= 1000 switch", counter)
    assert counter[-1] == 15 + 2 * L.LONG_PACKETS and z["sa_long"].max() >= 200


def main():
    lib = load()
    z = {}
    for n in L.FRAMES:
        z["sa_%d" % n], z["detail_%d" % n], z["state_%d" % n] = record(lib, n)
    z["sa_long"], z["state_long"], z["state_long_square"] = record_long(lib)
    check(z)
    np.savez_compressed(L.FIXTURE, **z)
    print("wrote %s: %d arrays, %d bytes" % (L.FIXTURE, len(z), os.path.getsize(L.FIXTURE)))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What the packed 16-bit sums meet on the input families of tests/test_gpu_dot_sites.py: the host build of the kernel source
(SX_NLANES == 1) compiled with -DSX_DOT_COUNT into build/, run over every 16 kHz family, counters printed per family (solo_fix.h,
SX_DOT_COUNTED).  The same build must reproduce the recorded reference output, which is checked too.

  python tools/debug/dot_branches.py          (profiles/dot_sites.txt, section 4)"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import dot_sites_inputs as B  # noqa: E402

lib_path = os.path.join(ROOT, "build", "libsolo_emu_dot_count.so")
os.makedirs(os.path.dirname(lib_path), exist_ok=True)
subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-fwrapv", "-fno-strict-aliasing", "-DSOLO_HOST_EMU", "-DSX_DOT_COUNT",
                       os.path.join(ROOT, "tests", "emu", "solo_emu.cpp"), "-o", lib_path])
lib = C.CDLL(lib_path)
lib.emu_enc_create.restype = C.c_void_p
lib.emu_enc_create.argtypes = [C.c_int, C.c_int]
lib.emu_enc_packet.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
lib.emu_enc_destroy.argtypes = [C.c_void_p]
count = (C.c_longlong * 16).in_dll(lib, "sx_dot_count")
z = np.load(os.path.join(ROOT, "tests", "golden", "dot_sites.npz"))
print("%-24s %15s %15s %13s %11s %17s %7s" % ("family", "stage-1 lags", "stage-2 lags", "winning lag", "shift > 0", "frames", "interp."))
print("%-24s %15s %15s %13s %11s %17s %7s" % ("", "even / odd", "even / odd", "even / odd", "4k / 8k", "voiced / unvoiced", "search"))
for name in B.FAMILIES:
    pcm = B.family(name)
    for i in range(16): count[i] = 0
    for s in range(B.N):
        h = lib.emu_enc_create(B.RATE, 0)
        for p in range(B.P):
            bits, nb = np.zeros(1100, np.uint8), np.zeros(2, np.int16)
            x = np.ascontiguousarray(pcm[s, p])
            n = lib.emu_enc_packet(h, x.ctypes.data, bits.ctypes.data, 1024, nb.ctypes.data)
            assert (int(nb[0]), int(nb[1])) == tuple(int(v) for v in z[name + "/nbytes"][s, p]) and n == nb[0], (name, s, p)
            assert np.array_equal(bits[:n], z[name + "/bits"][s, p, :n]), (name, s, p)
        lib.emu_enc_destroy(h)
    c = list(count)
    print("%-24s %15s %15s %13s %11s %17s %7d" % (name, "%d / %d" % (c[0], c[1]), "%d / %d" % (c[2], c[3]), "%d / %d" % (c[4], c[5]),
                                                  "%d / %d" % (c[6], c[7]), "%d / %d" % (c[8], c[9]), c[10]))

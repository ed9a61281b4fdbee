#!/usr/bin/env python3
"""Which branches of sx_burg_modified the input families of tests/test_gpu_burg_sites.py reach: the host build of the kernel source
(SX_NLANES == 1) compiled with -DSX_BURG_COUNT into build/, run over every family, counters printed per call site
(0: whole frame, 1: second half, 2: high band).  The same build must reproduce the recorded reference output, which is checked too.

  python tools/debug/burg_branches.py          (profiles/burg_steps.txt, section 4)"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import burg_sites_inputs as B  # noqa: E402

lib_path = os.path.join(ROOT, "build", "libsolo_emu_burg_count.so")
os.makedirs(os.path.dirname(lib_path), exist_ok=True)
subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-fwrapv", "-fno-strict-aliasing", "-DSOLO_HOST_EMU", "-DSX_BURG_COUNT",
                       os.path.join(ROOT, "tests", "emu", "solo_emu.cpp"), "-o", lib_path])
lib = C.CDLL(lib_path)
lib.emu_enc_create.restype = C.c_void_p
lib.emu_enc_create.argtypes = [C.c_int, C.c_int]
lib.emu_enc_packet.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
lib.emu_enc_destroy.argtypes = [C.c_void_p]
count = (C.c_longlong * 12).in_dll(lib, "sx_burg_count")
z = np.load(os.path.join(ROOT, "tests", "golden", "burg_sites.npz"))
print("%-26s %-12s %8s %10s %12s %s" % ("family", "site", "hi runs", "hi = false", "early exits", "second half accumulates like the whole frame"))
for name in B.FAMILIES:
    pcm = B.family(name)
    for i in range(12): count[i] = 0
    for s in range(B.N):
        h = lib.emu_enc_create(B.RATE, 0)
        for p in range(B.P):
            bits, nb = np.zeros(1100, np.uint8), np.zeros(2, np.int16)
            x = np.ascontiguousarray(pcm[s, p])
            n = lib.emu_enc_packet(h, x.ctypes.data, bits.ctypes.data, 1024, nb.ctypes.data)
            assert (int(nb[0]), int(nb[1])) == tuple(int(v) for v in z[name + "/nbytes"][s, p]) and n == nb[0], (name, s, p)
            assert np.array_equal(bits[:n], z[name + "/bits"][s, p, :n]), (name, s, p)
        lib.emu_enc_destroy(h)
    for site, label in enumerate(("whole frame", "second half", "high band")):
        c = count[4 * site:4 * site + 4]
        print("%-26s %-12s %8d %10d %12d %s" % (name, label, c[0], c[1], c[2], "%d of %d" % (c[3], c[0] + c[1]) if site == 1 else ""))

"""CPU half of tests/test_gpu_dot2_primitive.py: the host twins of sx_dot2 / sx_pair (solo_fix.h, probe ops 50 and 51 of the host
emulation) on the same operands, and the expectation itself on cases worked out by hand."""
import ctypes as C

import numpy as np

import dot2_operands as D
import solo_testlib as T


def _emu(op, a, b, c):
    emu = T.load_emu()
    emu.emu_l0.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    out = np.zeros(a.size, np.int32)
    emu.emu_l0(op, a.size, a.ctypes.data, b.ctypes.data, c.ctypes.data, out.ctypes.data)
    return out


def test_expectation_by_hand():
    m = D._pack([-32768], [-32768])
    assert D.dot2_expected(m, m, np.array([0], np.int32))[0] == -(1 << 31)            # 2 x 2^30 = 2^31 wraps to INT32_MIN
    assert D.dot2_expected(m, m, np.array([-1], np.int32))[0] == (1 << 31) - 1
    assert D.dot2_expected(D._pack([3], [-5]), D._pack([7], [11]), np.array([100], np.int32))[0] == 100 + 21 - 55
    assert D.pair_expected(np.array([0x11112222], np.int32), np.array([0x33334444], np.int32), np.array([1], np.int32))[0] == 0x44441111
    assert D.pair_expected(np.array([0x11112222], np.int32), np.array([0x33334444], np.int32), np.array([0], np.int32))[0] == 0x11112222


def test_host_twins():
    a, b, c = D.dot2_operands()
    assert np.array_equal(_emu(50, a, b, c), D.dot2_expected(a, b, c))
    lo, hi, par = D.pair_operands()
    assert np.array_equal(_emu(51, lo, hi, par), D.pair_expected(lo, hi, par))

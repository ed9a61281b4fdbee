"""sx_dot2 and sx_pair (solo_amd/csrc/solo_fix.h) as hipcc compiled them for gfx950, through the level-0 probe (solo_l0_probe.h, ops 50
and 51), in ONE launch each: acc + a.lo * b.lo + a.hi * b.hi must WRAP modulo 2^32 -- the instruction behind it (v_dot2_i32_i16 without
clamp) is used where the reference's SMLABB chains can pass 2^31 (two products of -32768 x -32768 already do), so a saturating or
otherwise different sum there would change payload bytes.  Expected values: int64 arithmetic in numpy, wrapped to 32 bits.
The CPU half (tests/test_dot2_primitive.py) runs the same operands through the host twins."""
import ctypes as C

import numpy as np
import pytest

import dot2_operands as D

pytestmark = pytest.mark.gpu


def _probe(op, a, b, c):
    import torch
    import solo_amd
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    lib = solo_amd.load_library()
    lib.solo_debug_l0.restype = C.c_int32
    lib.solo_debug_l0.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    da, db, dc = (torch.from_numpy(v).cuda() for v in (a, b, c))
    out = torch.zeros(a.size, dtype=torch.int32, device="cuda")
    assert lib.solo_debug_l0(op, a.size, da.data_ptr(), db.data_ptr(), dc.data_ptr(), out.data_ptr()) == 0
    return out.cpu().numpy()


def test_dot2_wraps_on_every_edge_combination_and_a_million_random_operands():
    a, b, c = D.dot2_operands()
    assert a.size >= 6 ** 4 * 5 + 1000000
    got, want = _probe(50, a, b, c), D.dot2_expected(a, b, c)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (bad.size, hex(int(a[bad[0]]) & 0xFFFFFFFF), hex(int(b[bad[0]]) & 0xFFFFFFFF), int(c[bad[0]]), int(got[bad[0]]), int(want[bad[0]]))


def test_pair_at_either_parity():
    lo, hi, par = D.pair_operands()
    got, want = _probe(51, lo, hi, par), D.pair_expected(lo, hi, par)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (bad.size, int(lo[bad[0]]), int(hi[bad[0]]), int(par[bad[0]]))

"""The wave-level vocabulary of solo_amd/csrc/solo_wave.h in its 64-lane form -- wv_sum, wv_max, wv_min, wv_row_sum, wv_col_sum,
wv_sum64, wv_scan_incl, wv_argmin, wv_argmax, wv_bcast, SX_UNI, SX_RDLANE / SX_WRLANE, sx_lcg_first / sx_lcg_next -- on the GPU
(probe: solo_debug_waveops, compiled in the translation unit of the decoder kernels) against the plain integer definitions of
tests/wave_model.py: exact equality in all 64 lanes of every result row.  The host emulation builds this vocabulary for one lane,
where it is the identity; this module is its only direct check.

mode 0 applies every primitive to the raw inputs of the families A (random), B (extremes, one-hot), C (ties inside and across the
16-lane rows, idx orders that disagree with the lane order), D (64-bit carries) and E (scan); mode 1 chains the primitives on each
other's results (the DPP read of a just-written register, straight and inside a loop of runtime trip count) on A, B and C.  Both
with one wavefront per workgroup and with four (the front kernel's geometry).  One launch per mode / geometry / family.

mode 2 is the workgroup vocabulary of the same header (wg_sum, wg_scan_incl, wg_total: the four vectors of a workgroup are its 256
lanes) on prefixes of A, B and E whose length is a multiple of four, and once on a length of 1 modulo 4, where three wavefronts of
the last workgroup have no vector: they contribute zeros, stay for the barriers and store nothing.

Not covered: the SX_GROUP (16-lane) forms of the same functions.  No kernel calls them (the quantiser has its own RW* exchanges,
tests/test_gpu_nsq_row.py)."""
import numpy as np
import pytest

import wave_model as M

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5AA5A5
CASES = [(0, fam) for fam in "ABCDE"] + [(1, fam) for fam in "ABC"]


# mode 2: (family, vectors): B's first half holds every one-hot lane and every extreme once
CASES_WG = [("A", 256), ("B", 580), ("E", 256), ("A", 257)]


def _run(mode, fam, wpb, n=None):
    import torch
    import solo_amd
    lib = solo_amd.load_library()
    names = (M.ROWS0, M.ROWS1, M.ROWS2)[mode]
    assert lib.solo_debug_waveops(mode, 0, wpb, None, None, None) == len(names)        # the probe's row count is the model's
    f = M.family(fam)
    n = f["v"].shape[0] if n is None else n
    d_v, d_aux = torch.from_numpy(f["v"][:n].copy()).cuda(), torch.from_numpy(f["aux"][:n].copy()).cuda()
    # (one vector's worth of guard words behind the output: the probe writes its own rows and nothing else)
    d_out = torch.full(((n + 1) * len(names) * 64,), SENTINEL, dtype=torch.int32, device="cuda")
    assert lib.solo_debug_waveops(mode, n, wpb, d_v.data_ptr(), d_aux.data_ptr(), d_out.data_ptr()) == len(names)
    got = d_out.cpu().numpy().reshape(n + 1, len(names), 64)
    assert (got[n] == SENTINEL).all(), "the probe wrote behind its output"
    return names, f, got[:n]


@pytest.mark.parametrize("wpb", [1, 4])
@pytest.mark.parametrize("mode,fam", CASES)
def test_wave_ops(mode, fam, wpb):
    names, f, got = _run(mode, fam, wpb)
    _compare(names, f, got, M.expected(mode, fam), "mode %d, family %s, %d waves per block" % (mode, fam, wpb))


@pytest.mark.parametrize("fam,n", CASES_WG)
def test_workgroup_ops(fam, n):
    assert n <= M.family(fam)["v"].shape[0] and (n % 4 == 0 or n % 4 == 1)
    names, f, got = _run(2, fam, 4, n)
    _compare(names, f, got, M.mode2(f["v"][:n]), "mode 2, family %s, %d vectors" % (fam, n))


def test_workgroup_ops_need_four_waves():
    import solo_amd
    assert solo_amd.load_library().solo_debug_waveops(2, 0, 1, None, None, None) == -1


def _compare(names, f, got, want, what):
    bad = got != want
    if bad.any():
        per_row = bad.any(axis=2).sum(axis=0)
        lines = ["%s: %d of %d vectors differ" % (what, int(bad.any(axis=(1, 2)).sum()), got.shape[0])]
        for r in np.nonzero(per_row)[0]:
            k = int(np.nonzero(bad[:, r].any(axis=1))[0][0])
            lanes = np.nonzero(bad[k, r])[0]
            l = int(lanes[0])
            lines.append("  %s: %d vectors; first: vector %d (%s) lane %d got %d want %d (%d lanes of it differ: %s)"
                         % (names[r], int(per_row[r]), k, f["tags"][k], l, int(got[k, r, l]), int(want[k, r, l]), len(lanes),
                            lanes.tolist() if len(lanes) <= 16 else "%d .. %d" % (lanes[0], lanes[-1])))
        pytest.fail("\n".join(lines), pytrace=False)

"""PCM resampler (solo_resample, solo_amd/csrc/solo_resample.h) without a GPU: the fixture recorded from the compiled reference
(tests/golden/resample.npz), the independent model of tests/resample_model.py and the host form of the kernel source (compiled by this
test from tests/resample_host.cpp, through tests/host_build.py) must agree sample for sample and state byte for state byte.  No tolerance anywhere."""
import ctypes as C
import os

import numpy as np
import pytest

import resample_lib as L
import resample_model as M
import solo_testlib as T
from host_build import host_lib

REF_LIB = os.path.join(T.ROOT, "oracle", "_ref", "libsolo_ref_fix.so")
CASES = [(fi, fo, 40) for fi, fo in L.PAIRS] + [(fi, fo, 20) for fi, fo in L.PAIRS_20MS]
ids = lambda c: "%d-%d-%dms" % (c[0] // 1000, c[1] // 1000, c[2])


@pytest.fixture(scope="module")
def host():
    lib = host_lib("resample")
    lib.emu_rs_run.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.emu_rs_call_ok.argtypes = [C.c_int] * 6 + [C.c_void_p, C.c_void_p]
    lib.emu_rs_list_ok.argtypes = [C.c_void_p, C.c_int, C.c_int]
    return lib


def host_run(lib, fs_in, fs_out, state, pcm, rows=None):
    """pcm int16 [n, P, L], state int32 [n_rows, 24] (updated in place) -> (status, out int16 [n, P, L'], count)"""
    n, P, Ls = pcm.shape
    outs = lib.emu_rs_out_samples(fs_in, fs_out, Ls)
    out = np.full((n, P, max(outs, 1)), 0x5A5A, dtype=np.int16)
    count = np.zeros(2, dtype=np.int32)
    pcm = np.ascontiguousarray(pcm)
    m = None if rows is None else np.ascontiguousarray(rows, dtype=np.int32)
    r = lib.emu_rs_run(fs_in, fs_out, state.shape[0], state.ctypes.data, None if m is None else m.ctypes.data, n, pcm.ctypes.data, P, Ls,
                       out.ctypes.data, count.ctypes.data)
    return r, out, count


def states_u8(state):
    return state.view(np.uint8).reshape(state.shape[0], L.STATE_BYTES)


# ---- the fixture holds what the tests rely on (checked against the fixture, not against code under test) ----
@pytest.mark.parametrize("pair", L.SATURATING, ids=lambda p: "%d-%d" % (p[0] // 1000, p[1] // 1000))
def test_fixture_white_noise_saturates(pair):
    pcm, _ = L.expected(*pair)
    sat = int(((pcm[0] >= 32767) | (pcm[0] == -32768)).sum())
    print("saturated output samples of family 0, %d -> %d: %d of %d" % (pair[0], pair[1], sat, pcm[0].size))
    assert sat > 0


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_fixture_zero_row_stays_zero(case):
    pcm, st = L.expected(*case)
    assert pcm.shape[0] == L.FAMILIES and st.shape == (L.FAMILIES, pcm.shape[1], L.STATE_BYTES)
    assert not pcm[5].any() and not st[5].any()
    assert pcm.shape[2] == case[0] // 1000 * case[2] * case[1] // case[0]


# ---- model == fixture ----
@pytest.mark.parametrize("case", CASES, ids=ids)
def test_model_equals_fixture(case):
    fs_in, fs_out, ms = case
    pcm, st = L.expected(*case)
    x = L.inputs(fs_in, ms)
    for f in range(L.FAMILIES):
        m = M.Model(fs_in, fs_out)
        for p in range(pcm.shape[1]):
            out = m.run(x[f, p])
            assert np.array_equal(out, pcm[f, p]), (case, f, p, "PCM")
            assert np.array_equal(m.state_bytes(), st[f, p]), (case, f, p, "state")


# ---- model == the compiled reference on inputs the fixture has not seen ----
@pytest.mark.skipif(not os.path.exists(REF_LIB), reason="the compiled reference is not built here")
@pytest.mark.parametrize("case", CASES, ids=ids)
def test_model_equals_reference_fresh_seed(case):
    import sys
    sys.path.insert(0, T.GOLDEN)
    import make_resample as G
    fs_in, fs_out, ms = case
    seed = 0x5EED0000 + fs_in // 1000 * 64 + fs_out // 1000
    pcm, st = G.record(G.load(), fs_in, fs_out, ms, seed)
    x = L.inputs(fs_in, ms, seed)
    for f in (0, 1, 3):                                     # the families the seed or the rate changes
        m = M.Model(fs_in, fs_out)
        for p in range(L.PACKETS):
            assert np.array_equal(m.run(x[f, p]), pcm[f, p]), (case, f, p, "PCM")
            assert np.array_equal(m.state_bytes(), st[f, p]), (case, f, p, "state")


# ---- the host form of the kernel source ----
@pytest.mark.parametrize("case", CASES, ids=ids)
def test_host_form_equals_fixture(host, case):
    fs_in, fs_out, ms = case
    pcm, st = L.expected(*case)
    x = L.inputs(fs_in, ms)
    state = np.zeros((L.FAMILIES, 24), dtype=np.int32)
    for p in range(pcm.shape[1]):                           # one packet per call, as the fixture was recorded
        r, out, _ = host_run(host, fs_in, fs_out, state, x[:, p:p + 1])
        assert r == 0
        assert np.array_equal(out[:, 0], pcm[:, p]), (case, p, "PCM")
        assert np.array_equal(states_u8(state), st[:, p]), (case, p, "state")


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_host_form_one_call_equals_four(host, case):
    fs_in, fs_out, ms = case
    pcm, st = L.expected(*case)
    x = L.inputs(fs_in, ms)
    state = np.zeros((L.FAMILIES, 24), dtype=np.int32)
    r, out, _ = host_run(host, fs_in, fs_out, state, x)
    assert r == 0
    assert np.array_equal(out[:, :pcm.shape[1]], pcm)
    if pcm.shape[1] == L.PACKETS:
        assert np.array_equal(states_u8(state), st[:, -1])


def test_host_form_more_rows_than_a_group_and_a_list(host):
    """rows beyond one group, and a listed subset: compact I/O, the unlisted rows' state untouched, a bad list refused"""
    fs_in, fs_out = 48000, 32000
    R = host.emu_rs_rows_per_group()
    n = 2 * R + 3
    pcm, st = L.expected(fs_in, fs_out)
    x = L.tiled(L.inputs(fs_in), n)
    state = np.zeros((n, 24), dtype=np.int32)
    r, out, count = host_run(host, fs_in, fs_out, state, x[:, :2])
    assert r == 0 and list(count) == [n, n]
    assert np.array_equal(out, L.tiled(pcm, n)[:, :2]) and np.array_equal(states_u8(state), L.tiled(st, n)[:, 1])
    rows = np.arange(0, n, 3, dtype=np.int32)
    before = state.copy()
    r, out, count = host_run(host, fs_in, fs_out, state, x[rows, 2:3], rows)
    assert r == 0 and list(count) == [len(rows), len(rows)]
    assert np.array_equal(out[:, 0], L.tiled(pcm, n)[rows, 2])
    rest = np.setdiff1d(np.arange(n), rows)
    assert np.array_equal(state[rest], before[rest])
    for bad in ([3, 2, 5], [0, 1, n]):
        keep = state.copy()
        r, out, count = host_run(host, fs_in, fs_out, state, x[:3, 3:4], bad)
        assert r == -2 and count[0] == -1
        assert np.all(out == 0x5A5A) and np.array_equal(state, keep)


# ---- what the host refuses before anything is enqueued ----
def test_unsupported_pairs_are_refused(host):
    rates = sorted(set(L.RATES) | {11025, 12000, 22050, 24000, 44100, 96000})
    offered = set(L.PAIRS)
    for fi in rates:
        for fo in rates:
            assert host.emu_rs_supported(fi, fo) == (1 if (fi, fo) in offered else 0), (fi, fo)
            assert M.supported(fi, fo) == ((fi, fo) in offered)
    for fi, fo in ((16000, 16000), (32000, 8000), (48000, 8000), (8000, 32000), (8000, 48000), (44100, 16000), (96000, 48000), (0, 16000), (-16000, 16000)):
        assert host.emu_rs_supported(fi, fo) == 0, (fi, fo)


def test_in_samples_off_the_grid_and_n_out_of_range_are_refused(host):
    buf = np.zeros(64, dtype=np.int16)
    a = (buf.ctypes.data + 15) & ~15
    far = a + (1 << 32)                                     # (never dereferenced: the checks look at addresses only)
    for fs_in, fs_out in L.PAIRS:
        g = fs_in // 100
        for ms in (10, 20, 40, 60):
            assert host.emu_rs_out_samples(fs_in, fs_out, g * ms // 10) == fs_out // 100 * ms // 10
        for bad in (0, -g, g - 1, g + 1, g // 2, 3 * g + 8):
            assert host.emu_rs_out_samples(fs_in, fs_out, bad) == -1
            assert host.emu_rs_call_ok(fs_in, fs_out, 8, 8, 1, bad, a, far) == 0
        assert host.emu_rs_call_ok(fs_in, fs_out, 8, 8, 1, 4 * g, a, far) == 1
        for n in (0, -1, 9):
            assert host.emu_rs_call_ok(fs_in, fs_out, 8, n, 1, 4 * g, a, far) == 0
        assert host.emu_rs_call_ok(fs_in, fs_out, 8, 8, 0, 4 * g, a, far) == 0
        assert host.emu_rs_call_ok(fs_in, fs_out, 8, 8, 1, 4 * g, None, far) == 0 and host.emu_rs_call_ok(fs_in, fs_out, 8, 8, 1, 4 * g, a, None) == 0
        assert host.emu_rs_call_ok(fs_in, fs_out, 8, 8, 1, 4 * g, a + 2, far) == 0 and host.emu_rs_call_ok(fs_in, fs_out, 8, 8, 1, 4 * g, a, far + 8) == 0
        assert host.emu_rs_call_ok(fs_in, fs_out, 8, 8, 1, 4 * g, a, a + 16) == 0                     # overlap
        assert host.emu_rs_call_ok(fs_in, fs_out, 1 << 20, 1 << 20, 64, 4 * g, a, far + (1 << 40)) == 0     # 2^31 elements and more
    rows = lambda v: np.array(v, dtype=np.int32).ctypes.data
    assert host.emu_rs_list_ok(rows([0, 2]), 2, 4) == 1 and host.emu_rs_list_ok(rows([2, 0]), 2, 4) == 1
    assert host.emu_rs_list_ok(rows([0, 0]), 2, 4) == 0 and host.emu_rs_list_ok(rows([0, 4]), 2, 4) == 0 and host.emu_rs_list_ok(rows([-1]), 1, 4) == 0
    assert host.emu_rs_list_ok(rows([0, 1, 2, 3, 0]), 5, 4) == 0 and host.emu_rs_list_ok(None, 1, 4) == 0 and host.emu_rs_list_ok(rows([0]), 0, 4) == 0

"""Mixing bridge (solo_mix, solo_amd/csrc/solo_mix.h) without a GPU: the room plan and the per-(room, packet) walk are compiled for the
host by this test (tests/mix_host.cpp, through tests/host_build.py) and compared with the independent numpy model of
tests/mix_model.py -- every output sample, the energies, the flags and the count."""
import ctypes as C

import numpy as np
import pytest

from host_build import host_lib
from mix_model import GAINS, mix_case, model_mix, ties_decide

FILL_O, FILL_E, FILL_M = 0x1234, -77, 0xA5
GUARD = 3                                                         # rows behind the call's


@pytest.fixture(scope="module")
def host():
    lib = host_lib("mix")
    lib.emu_mix.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.emu_mix_before.argtypes = [C.c_longlong, C.c_int, C.c_longlong, C.c_int]
    lib.emu_mix_contrib.argtypes = [C.c_int, C.c_int]
    return lib


def aligned(shape, dtype, fill=0):
    """an array whose first byte is 16-byte aligned (the interface's rule for PCM)"""
    nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
    raw = np.zeros(nbytes + 16, np.uint8)
    off = (-raw.ctypes.data) % 16
    a = raw[off:off + nbytes].view(dtype).reshape(shape)
    a[...] = fill
    return a


def run_host(host, pcm, room, n_rooms, gain, max_speakers, with_side=True, with_count=True):
    n, P, L = pcm.shape
    x = aligned(pcm.shape, np.int16)
    x[...] = pcm
    out = aligned((n + GUARD, P, L), np.int16, FILL_O)
    energy = np.full((n + GUARD, P), FILL_E, np.int64)
    mixed = np.full((n + GUARD, P), FILL_M, np.uint8)
    cnt = np.full(4, 0x5A5A5A5A, np.int32)
    room = np.ascontiguousarray(room, np.int32)
    p = lambda a: a.ctypes.data if a is not None else None
    ret = host.emu_mix(p(x), n, P, L, p(room), n_rooms, p(gain), max_speakers, p(out), p(energy) if with_side else None,
                       p(mixed) if with_side else None, p(cnt) if with_count else None)
    count = dict(rows=int(cnt[0]), rooms=int(cnt[1]), clipped=int(cnt[2:4].view(np.int64)[0]))
    return ret, out, energy, mixed, count, cnt


def compare(got, want, n):
    ret, out, energy, mixed, count, _ = got
    assert ret == 0
    assert count == want["count"], (count, want["count"])
    bad = np.argwhere((out != want["out"]).any(axis=2))
    assert len(bad) == 0, bad[:8].tolist()
    assert np.array_equal(energy, want["energy"])
    assert np.array_equal(mixed, want["mixed"])
    assert (out[n:] == FILL_O).all() and (energy[n:] == FILL_E).all() and (mixed[n:] == FILL_M).all()


def fills(n, P, L):
    return dict(out=np.full((n + GUARD, P, L), FILL_O, np.int16), energy=np.full((n + GUARD, P), FILL_E, np.int64),
                mixed=np.full((n + GUARD, P), FILL_M, np.uint8))


def model(pcm, room, n_rooms, gain, max_speakers):
    n, P, L = pcm.shape
    f = fills(n, P, L)
    pad = lambda a: np.concatenate([a, np.zeros((GUARD,) + a.shape[1:], a.dtype)])
    w = model_mix(pad(pcm), np.concatenate([room, np.full(GUARD, -1, np.int32)]), n_rooms, None if gain is None else pad(gain), max_speakers, **f)
    return w


def check_case_has_everything(pcm, room, gain):
    sizes = set(np.bincount(room[room >= 0]).tolist())
    assert {1, 2, 3, 64, 65} <= sizes and any(900 <= s <= 1100 for s in sizes), sizes
    assert (room == -1).sum() >= 10
    assert set(GAINS) <= set(gain.tolist())
    assert (np.abs(pcm.astype(np.int32)).min(axis=(1, 2)) >= 32767).sum() >= 10         # full-scale rows


def test_count_struct_is_16_bytes(host):
    import solo_amd
    assert host.emu_mix_count_size() == 16 == C.sizeof(solo_amd.solo_mix_count_t)


def test_contribution_and_order(host):
    for x, g, want in [(1000, 4096, 1000), (-1000, 4096, -1000), (-32768, 4096, -32768), (32767, 32767, 262128), (-32768, 32767, -262136),
                       (1, 2048, 1), (-1, 2048, 0), (3, 2048, 2), (-3, 2048, -1), (12345, 0, 0), (-7, 1, 0)]:
        assert host.emu_mix_contrib(x, g) == want == (x * g + 2048) >> 12, (x, g)
    assert host.emu_mix_before(5, 9, 4, 1) == 1 and host.emu_mix_before(4, 1, 5, 9) == 0
    assert host.emu_mix_before(5, 1, 5, 9) == 1 and host.emu_mix_before(5, 9, 5, 1) == 0 and host.emu_mix_before(5, 3, 5, 3) == 0
    assert host.emu_mix_before(2 ** 40, 7, 2 ** 40 - 1, 0) == 1


@pytest.mark.parametrize("L", [320, 640, 1280])
@pytest.mark.parametrize("max_speakers", [0, 1, 3, 64])
def test_host_mix_against_model(host, L, max_speakers):
    P = 3
    pcm, room, gain, n_rooms = mix_case(100 + L, P, L)
    check_case_has_everything(pcm, room, gain)
    n = pcm.shape[0]
    want = model(pcm, room, n_rooms, gain, max_speakers)
    assert want["count"]["clipped"] > 0 and want["count"]["rows"] == int((room >= 0).sum()) and want["count"]["rooms"] == len(set(room[room >= 0].tolist()))
    if max_speakers in (1, 3, 64):
        assert ties_decide(want["energy"][:n], room, max_speakers) > 0          # the row index decided somewhere
        assert 0 < want["mixed"][:n][room >= 0].sum() < (room >= 0).sum() * P
    # the cache boundary of the walk lies inside the case: rooms of exactly, and of one more than, what the cache holds
    sizes = set(np.bincount(room[room >= 0]).tolist())
    assert {host.emu_mix_cache_rows(L), host.emu_mix_cache_rows(L) + 1} <= sizes
    compare(run_host(host, pcm, room, n_rooms, gain, max_speakers), want, n)


@pytest.mark.parametrize("max_speakers", [0, 3])
def test_host_mix_without_gain_side_outputs_or_count(host, max_speakers):
    P, L = 2, 640
    pcm, room, gain, n_rooms = mix_case(7, P, L)
    n = pcm.shape[0]
    want = model(pcm, room, n_rooms, None, max_speakers)
    compare(run_host(host, pcm, room, n_rooms, None, max_speakers), want, n)
    ret, out, energy, mixed, count, cnt = run_host(host, pcm, room, n_rooms, None, max_speakers, with_side=False, with_count=False)
    assert ret == 0 and np.array_equal(out, want["out"])
    assert (energy == FILL_E).all() and (mixed == FILL_M).all() and (cnt == 0x5A5A5A5A).all()


def test_unity_two_member_rooms(host):
    """NULL gain, every member mixed: each row's output is the other row's input, exactly"""
    rng = np.random.default_rng(5)
    n, P, L = 64, 4, 640
    pcm = rng.integers(-32768, 32768, (n, P, L)).astype(np.int16)
    room = (rng.permutation(n) // 2).astype(np.int32)
    ret, out, energy, mixed, count, _ = run_host(host, pcm, room, n // 2, None, 0)
    other = np.empty(n, np.int64)
    for r in range(n // 2):
        a, b = np.flatnonzero(room == r)
        other[a], other[b] = b, a
    assert ret == 0 and np.array_equal(out[:n], pcm[other]) and count == dict(rows=n, rooms=n // 2, clipped=0)
    assert (mixed[:n] == 1).all() and np.array_equal(energy[:n], (pcm.astype(np.int64) ** 2).sum(axis=2))


@pytest.mark.parametrize("bad", [-2, 31, 2 ** 31 - 1, -2 ** 31])
def test_bad_room_id_refuses_the_call(host, bad):
    P, L = 2, 320
    pcm, room, gain, n_rooms = mix_case(9, P, L, sizes=(1, 2, 3, 9), loose=4)
    assert n_rooms == 11
    room = room.copy()
    room[5] = bad if bad != 31 else n_rooms
    ret, out, energy, mixed, count, cnt = run_host(host, pcm, room, n_rooms, gain, 3)
    assert ret == -1 and cnt[0] == -1 and (cnt[1:] == 0x5A5A5A5A).all()
    assert (out == FILL_O).all() and (energy == FILL_E).all() and (mixed == FILL_M).all()
    want = model_mix(pcm, room, n_rooms, gain, 3)
    assert want["count"]["rows"] == -1

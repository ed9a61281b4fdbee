"""Play-out time scaling (solo_timescale, solo_amd/csrc/solo_timescale.h) without a GPU: the row walk is compiled for the host by this test
(tests/timescale_host.cpp, through tests/host_build.py) and compared with the independent numpy model of tests/timescale_model.py
-- every output sample, shift, cost and the count, for every (in_packets, out_packets) in 1..4 x 1..4 at the four packet geometries -- and
with what the interface promises whatever the model says; then the model alone: the search must earn its keep on speech, and the
look-ahead term of the block before the last must lower the cost of the pinned last splice."""
import ctypes as C

import numpy as np
import pytest

from host_build import host_lib
from timescale_model import (FAMILIES, GEOMETRIES, PERIODS, geometry, lag_range, model_timescale, narrowest_window, nominal, speech_segments,
                             timescale_rows)

FILL_O, FILL_S, FILL_C, FILL_N = 0x1234, -77, -99, 0x5A5A5A5A
GUARD = 3                                                         # rows behind the call's
N = 67
RATIOS = ((2, 1), (3, 2), (1, 2), (2, 3))


@pytest.fixture(scope="module")
def host():
    lib = host_lib("timescale")
    lib.emu_timescale.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.emu_ts_sad.restype = lib.emu_ts_straddle.restype = C.c_uint
    lib.emu_ts_sad.argtypes = [C.c_uint] * 3
    lib.emu_ts_straddle.argtypes = [C.c_uint] * 2
    return lib


def aligned(shape, dtype, fill=0):
    """an array whose first byte is 16-byte aligned (the interface's rule for PCM)"""
    nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
    raw = np.zeros(nbytes + 16, np.uint8)
    off = (-raw.ctypes.data) % 16
    a = raw[off:off + nbytes].view(dtype).reshape(shape)
    a[...] = fill
    return a


def run_host(host, pcm, b, fs, with_shift=True, with_cost=True, with_count=True):
    n, a, L = pcm.shape
    M = geometry(fs, L, a, b)["M"]
    x = aligned(pcm.shape, np.int16)
    x[...] = pcm
    out = aligned((n + GUARD, b, L), np.int16, FILL_O)
    shift, cost = np.full((n + GUARD, M), FILL_S, np.int32), np.full((n + GUARD, M), FILL_C, np.int32)
    cnt = np.full(4, FILL_N, np.int32)
    ret = host.emu_timescale(x.ctypes.data, n, a, b, fs, L, out.ctypes.data, shift.ctypes.data if with_shift else None,
                             cost.ctypes.data if with_cost else None, cnt.ctypes.data if with_count else None)
    assert (x == pcm).all()
    return ret, out, shift, cost, dict(rows=int(cnt[0]), blocks=int(cnt[1]), cost=int(cnt[2:4].view(np.int64)[0])), cnt


def check_properties(pcm, fam, fs, b, out, shift, cost):
    """what the interface promises, whatever the model says"""
    n, a, L = pcm.shape
    g = geometry(fs, L, a, b)
    H, Li, Lo, M = g["H"], g["Li"], g["Lo"], g["M"]
    x, y = pcm.reshape(n, Li), out.reshape(n, Lo)
    assert np.array_equal(y[:, :H], x[:, :H]) and np.array_equal(y[:, -1], x[:, -1])
    assert (shift[:, 0] == 0).all() and (cost[:, 0] == 0).all() and (shift[:, M - 1] == 0).all()
    for m in range(1, M - 1):
        lo, hi = lag_range(m, Li, H, M)
        assert (shift[:, m] >= lo).all() and (shift[:, m] <= hi).all(), m
    assert (cost >= 0).all() and (cost <= 2 * H * 65535).all()
    if a == b:
        assert np.array_equal(y, x) and (shift == 0).all() and (cost == 0).all()
    # silence and constants: every candidate ties, the lag is the clipped 0, the output is the constant
    const = fam == FAMILIES.index("constant")
    assert (y[const] == x[const][:, :1]).all() and (cost[const] == 0).all()
    for m in range(1, M - 1):
        lo, hi = lag_range(m, Li, H, M)
        assert (shift[const, m] == min(max(0, lo), hi)).all()
    # a period that divides what is taken out or put in comes out as the same periodic signal
    per = np.flatnonzero(fam == FAMILIES.index("periodic"))[:len(PERIODS)]
    if a != b:
        for i, Tp in zip(per, PERIODS):
            assert ((a - b) * L) % Tp == 0 and np.array_equal(x[i], x[i, :Tp][np.arange(Li) % Tp])
            assert np.array_equal(y[i], x[i, :Tp][np.arange(Lo) % Tp]), (i, Tp)
            assert (cost[i] == 0).all()


def test_vocabulary(host):
    import solo_amd
    assert host.emu_ts_count_size() == 16 == C.sizeof(solo_amd.solo_timescale_count_t)
    for d in range(-240, 241):
        r = host.emu_ts_rank(d)
        assert r == 2 * abs(d) - (d < 0) and host.emu_ts_unrank(r) == d and 0 <= r <= 480
    assert host.emu_ts_sad(0xFFFF0000, 0x0000FFFF, 7) == 2 * 65535 + 7 and host.emu_ts_sad(0x80017FFF, 0x7FFF8001, 0) == 4
    assert host.emu_ts_straddle(0x44443333, 0x22221111) == 0x33332222
    for fs, L in GEOMETRIES:
        for a in range(1, 5):
            for b in range(1, 5):
                g = geometry(fs, L, a, b)
                assert host.emu_ts_nominal(0, g["Li"], g["H"], g["M"]) == 0 and host.emu_ts_nominal(g["M"] - 1, g["Li"], g["H"], g["M"]) == g["Li"] - g["H"]
                assert all(host.emu_ts_nominal(m, g["Li"], g["H"], g["M"]) == nominal(m, g["Li"], g["H"], g["M"]) for m in range(g["M"]))
                assert host.emu_ts_lds_bytes(g["Li"]) % 16 == 0 and host.emu_ts_lds_bytes(g["Li"]) <= 10240 + 32 + 384
    # the narrowest clipped window of all cases still holds every period the periodic rows are tested with
    w = narrowest_window([(fs, L, a, b) for fs, L in GEOMETRIES for a in range(1, 5) for b in range(1, 5)])
    print("narrowest clipped window: %d candidates" % w)
    assert max(PERIODS) <= w


@pytest.mark.parametrize("fs,L", GEOMETRIES)
def test_host_against_model(host, fs, L):
    by_abs = by_sign = 0
    for a in range(1, 5):
        for b in range(1, 5):
            pcm, fam = timescale_rows(100 * a + b, N, fs, L, a, b)
            assert all((fam == k).sum() >= N // 6 for k in range(len(FAMILIES))), np.bincount(fam)
            want = model_timescale(pcm, b, fs)
            ret, out, shift, cost, count, _ = run_host(host, pcm, b, fs)
            assert ret == 0 and count == want["count"], (a, b, count, want["count"])
            bad = np.argwhere((out[:N] != want["out"]).any(axis=2))
            assert len(bad) == 0, (a, b, bad[:8].tolist())
            assert np.array_equal(shift[:N], want["shift"]) and np.array_equal(cost[:N], want["cost"]), (a, b)
            assert (out[N:] == FILL_O).all() and (shift[N:] == FILL_S).all() and (cost[N:] == FILL_C).all()
            check_properties(pcm, fam, fs, b, out[:N], shift[:N], cost[:N])
            ties = (fam == FAMILIES.index("constant")) | (fam == FAMILIES.index("periodic"))
            by_abs += int(want["by_abs"][ties].sum())
            by_sign += int(want["by_sign"][ties].sum())
            sq = cost[:N][fam == FAMILIES.index("square")]
            if (a, b) == (4, 1):    # the +-full-scale row built for it (worst_square) reaches the bound of a cost, and nothing wraps: at 4 -> 1
                                    # the nominal positions are more than 4H apart, so the template of block M - 2 ends before its first candidate
                assert sq.max() == 2 * (fs // 200) * 65535, (a, b, int(sq.max()))
    print("%d Hz, %d samples: |lag| decided %d ties, the sign %d" % (fs, L, by_abs, by_sign))
    assert by_abs > 0 and by_sign > 0


@pytest.mark.parametrize("a,b", [(2, 1), (1, 2), (3, 3)])
def test_host_without_side_outputs_or_count(host, a, b):
    fs, L = 16000, 640
    pcm, fam = timescale_rows(7, 13, fs, L, a, b)
    want = model_timescale(pcm, b, fs)
    for ws, wc, wn in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
        ret, out, shift, cost, count, cnt = run_host(host, pcm, b, fs, with_shift=ws, with_cost=wc, with_count=wn)
        assert ret == 0 and np.array_equal(out[:13], want["out"]) and (out[13:] == FILL_O).all()
        assert np.array_equal(shift[:13], want["shift"]) if ws else (shift == FILL_S).all()
        assert np.array_equal(cost[:13], want["cost"]) if wc else (cost == FILL_C).all()
        assert count == want["count"] if wn else (cnt == FILL_N).all()


def test_host_refusals(host):
    fs, L, n = 16000, 640, 4
    x = aligned((n + 1, 2, L), np.int16)
    out = aligned((n, 4, L), np.int16, FILL_O)

    def call(pin=x.ctypes.data, n=n, a=2, b=1, fs=fs, L=L, pout=out.ctypes.data):
        return host.emu_timescale(pin, n, a, b, fs, L, pout, None, None, None)

    assert call() == 0
    out[...] = FILL_O
    assert call(pin=None) == -1 and call(pout=None) == -1 and call(n=0) == -1 and call(n=-1) == -1
    assert call(a=0) == -1 and call(a=5) == -1 and call(b=0) == -1 and call(b=5) == -1
    assert call(n=-(-2 ** 31 // (2 * L))) == -1 and call(n=-(-2 ** 31 // (4 * L)), b=4) == -1     # n x max(a, b) x L reaches 2^31
    assert call(fs=8000) == -1 and call(fs=48000) == -1 and call(L=1281) == -1 and call(fs=32000, L=400) == -1
    assert call(pin=x.ctypes.data + 2) == -1 and call(pout=out.ctypes.data + 8) == -1          # not 16-byte aligned
    assert call(pout=x.ctypes.data) == -1                                                       # in place
    assert call(pout=x.ctypes.data + (n * 2 - 1) * L * 2) == -1 and call(pin=out.ctypes.data + (n - 1) * L * 2) == -1      # overlapping by a packet
    assert (out == FILL_O).all()


@pytest.fixture(scope="module")
def speech_runs():
    """the speech family through the model, searched / pinned at the clipped nominal / searched without the look-ahead term: computed once.
    The segments are ALL those of the recording (cut back to back, mean |x| >= 200; no choice is made), at the recording's own rate."""
    runs = {}
    for fs, L in GEOMETRIES[:2]:
        for a, b in RATIOS:
            pcm = speech_segments(a * L)
            pcm = pcm.reshape(len(pcm), a, L)
            assert len(pcm) >= 50 and (np.abs(pcm.astype(np.int64)).mean(axis=(1, 2)) >= 200).all()
            runs[fs, L, a, b] = (model_timescale(pcm, b, fs), model_timescale(pcm, b, fs, search=False), model_timescale(pcm, b, fs, lookahead=False))
    return runs


def test_the_search_earns_its_keep(speech_runs):
    """Summed cost of the searched splices: at most 1/4 of the same model with every lag pinned at the clipped nominal, for 2 -> 1, 3 -> 2,
    1 -> 2 and 2 -> 3 on the recording at its own rate and the library's default packet (16 kHz, 40 ms: L = 640).  Found: 4.1 x, 7.2 x,
    6.1 x, 11.4 x.  The same at 20 ms packets (L = 320) is printed, not asserted: 2.9 x, 5.0 x, 3.8 x, 6.9 x -- 2 -> 1 has only M = 4
    blocks there, two of them searched, and the second of the two also carries the look-ahead term, which no lag can make small together
    with its splice; so the bound of 4 that was set with 40 ms packets in mind is not met by 2 -> 1 and 1 -> 2 at 20 ms."""
    for (fs, L, a, b), (full, pinned, _) in speech_runs.items():
        ratio = pinned["searched_cost"] / max(full["searched_cost"], 1)
        print("%d Hz, L %d, %d -> %d: %d rows, searched %d, pinned %d: %.1f x" % (fs, L, a, b, full["count"]["rows"], full["searched_cost"],
                                                                            pinned["searched_cost"], ratio))
        if L == 640:
            assert 4 * full["searched_cost"] <= pinned["searched_cost"], (fs, L, a, b, ratio)


def test_the_look_ahead_term_is_present(speech_runs):
    """mean cost of the pinned last splice: lower with the second term of block M - 2 than without it (found: 21 .. 74 k against 136 .. 173 k)"""
    for (fs, L, a, b), (full, _, blind) in speech_runs.items():
        n = full["count"]["rows"]
        print("%d Hz, L %d, %d -> %d: last splice %.0f with the look-ahead, %.0f without" % (fs, L, a, b, full["last_cost"] / n, blind["last_cost"] / n))
        assert full["last_cost"] < blind["last_cost"], (fs, L, a, b)

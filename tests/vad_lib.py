"""Inputs, fixture access and generated cases of the VAD tests (tests/test_vad_model.py, tests/test_vad_abi.py, tests/test_gpu_vad.py).

The PCM rows come from the speech fixture and from a pure-integer generator written out here (a 32-bit LCG, no library RNG), so the
fixture (tests/golden/vad.npz, written by tests/golden/make_vad.py from the compiled reference) holds expected outputs and states only.
Six rows of PACKETS packets of PACKET samples:

    0  tests/golden/Ch_f1_raw.pcm from sample 0: silence, onset, speech
    1  stationary noise, sigma about 100 (the sum of four uniform integers)
    2  a full-scale square wave of period 32: 500 Hz and its odd harmonics at 16 kHz, energy in all four bands (drives every band's
       noise level to its ceiling; with period 16 nothing falls below 1 kHz and band 0 stops short of it)
    3  all zeros
    4  row 0 shifted right by 6 bits (the small-energy branches)
    5  8 packets of loud noise, then zeros (speech_nrg <= 0: the halving of the activity)

and one long row of LONG_PACKETS packets (LONG_SQUARE packets of the square wave, then speech at half scale, repeated, over a little
noise), which runs past the counter >= 1000 switch of the noise tracker.  Its opening is there because the noise tracker cannot reach
its ceiling within row 2 at frames of 320 samples: from the state of SKP_Silk_VAD_Init the inverse noise level falls by at most
min_coef / 65536 of itself per frame, min_coef = 32767 / ((counter >> 4) + 1), which takes it from 2^31 / 1200 (band 3) to no less
than about 580 in 32 frames, and the ceiling 0x00FFFFFF needs 128 or less.  At frames of 160 samples row 2 has 64 frames and gets there.
"""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "vad.npz")
SPEECH = os.path.join(ROOT, "tests", "golden", "Ch_f1_raw.pcm")

FRAMES = (320, 160)
ROWS = 6
PACKETS = 16
PACKET = 640
LONG_PACKETS = 520
LONG_SQUARE = 48
LONG_KEPT = 32                                              # states of the long row are recorded after each of its last 32 packets
REF_BYTES = 112
STATE_BYTES = 128
SEED = 20241019


def lcg(seed, n):
    """n successive values of x -> 1664525 x + 1013904223 (mod 2^32), as a uint32 array (computed with Python ints)"""
    out, x = np.empty(n, dtype=np.uint32), seed & 0xFFFFFFFF
    for i in range(n):
        x = (1664525 * x + 1013904223) & 0xFFFFFFFF
        out[i] = x
    return out


def noise(seed, n, half):
    """sum of four uniform integers of [-half, half]: variance 4 half (half + 1) / 3"""
    r = (lcg(seed, 4 * n).astype(np.int64) >> 16) % (2 * half + 1) - half
    return r.reshape(n, 4).sum(axis=1)


def speech():
    return np.fromfile(SPEECH, dtype="<i2").astype(np.int64)


_inputs = {}


def inputs(seed=SEED):
    """int16 [ROWS, PACKETS, PACKET]"""
    if seed not in _inputs:
        n = PACKETS * PACKET
        sp = speech()[:n]
        i = np.arange(n)
        rows = [sp, noise(seed + 1, n, 87), np.where(i % 32 < 16, 32767, -32768), np.zeros(n, dtype=np.int64), sp >> 6,
                np.where(i < 8 * PACKET, noise(seed + 5, n, 4000), 0)]
        a = np.stack(rows)
        assert a.min() >= -32768 and a.max() <= 32767
        _inputs[seed] = a.astype(np.int16).reshape(ROWS, PACKETS, PACKET)
    return _inputs[seed]


def long_input(seed=SEED):
    """int16 [LONG_PACKETS, PACKET]"""
    key = ("long", seed)
    if key not in _inputs:
        n = LONG_PACKETS * PACKET
        sp = speech()
        a = (np.resize(sp, n) >> 1) + noise(seed + 9, n, 26)
        a[:LONG_SQUARE * PACKET] = np.where(np.arange(LONG_SQUARE * PACKET) % 32 < 16, 32767, -32768)
        assert a.min() >= -32768 and a.max() <= 32767
        _inputs[key] = a.astype(np.int16).reshape(LONG_PACKETS, PACKET)
    return _inputs[key]


_fixture = None


def fixture():
    """sa_<N> uint8 [ROWS, PACKETS, F], detail_<N> int32 [ROWS, PACKETS, F, 6], state_<N> uint8 [ROWS, PACKETS, 112] for N in FRAMES;
    sa_long uint8 [LONG_PACKETS, 2], state_long uint8 [LONG_KEPT, 112], state_long_square uint8 [112] (after packet LONG_SQUARE - 1), at
    frame 320"""
    global _fixture
    if _fixture is None:
        _fixture = dict(np.load(FIXTURE))
    return _fixture


def init_state(n_rows):
    """uint8 [n_rows, 128]: what SKP_Silk_VAD_Init leaves, selection state zero (written out here, not taken from code under test)"""
    w = np.zeros(32, dtype=np.int32)
    w[10:14] = 25600
    bias = np.array([50, 25, 16, 12], dtype=np.int32)
    w[15:19] = 100 * bias
    w[19:23] = 0x7FFFFFFF // (100 * bias)
    w[23:27] = bias
    w[27] = 15
    return np.tile(w.view(np.uint8), (n_rows, 1))


# ---- generated cases of the selection ----------------------------------------------------------------------------------------------------
def select_streams(seed, n, P, F):
    """sa uint8 [n, P, F] and level uint8 [n, P]: activities that cross both thresholds in runs, levels in a narrow band so that keys tie"""
    r = lcg(seed, n * P * (F + 2)).astype(np.int64).reshape(n, P, F + 2) >> 12
    run = (np.arange(P)[None, :] // 3 + r[:, :1, 0] % 5) % 4                    # 0, 1: quiet, 2: in between, 3: loud -- runs of 3 packets
    base = np.array([10, 40, 100, 200])[run]
    sa = np.clip(base[:, :, None] + r[:, :, :F] % 41 - 20, 0, 255)
    level = 30 + r[:, :, F] % 4 + np.where(r[:, :, F + 1] % 16 == 0, 100, 0)    # a few far-away packets (level 130 .. 133 counts as 127)
    return sa.astype(np.uint8), level.astype(np.uint8)


def select_rooms(n, sizes, seed):
    """room ids int32 [n]: rooms of the given sizes dealt over the rows in a shuffled order, the rest in no room (-1)"""
    assert sum(sizes) <= n
    order = np.argsort(lcg(seed, n), kind="stable")
    room = np.full(n, -1, dtype=np.int32)
    at = 0
    for r, s in enumerate(sizes):
        room[order[at:at + s]] = r
        at += s
    return room


SELECT_SIZES = (1, 2, 3, 65, 200, 0)                        # members of rooms 0 .. 5 (room 5 is empty)
SELECT_N = 280                                              # 271 rows in rooms, 9 in none
SELECT_P = 12
SELECT_F = 2
SELECT_PARAMS = [dict(max_speakers=ms, on=128, off=64, hang=hang, stick=stick) for ms in (1, 3, 64) for hang in (0, 3) for stick in (0, 6)]


def select_case(seed=SEED):
    sa, level = select_streams(seed + 20, SELECT_N, SELECT_P, SELECT_F)
    room = select_rooms(SELECT_N, SELECT_SIZES, seed + 21)
    gain = ((lcg(seed + 22, SELECT_N).astype(np.int64) >> 16) % 9000 - 500).astype(np.int16)      # some negative: they count as 0
    return sa, level, room, gain


def tie_case():
    """one room of 6 rows, all active, level 40 (key 87) unless set below; for max_speakers 2, stick 6, hang 0 -> TIE_EXPECTED:
    packet 0: six equal newcomers, the smaller positions win; 1: the incumbents at 93; 2: newcomer 5 at 93 ties with them and loses to
    s = 1; 3: newcomer 5 at 94 comes first, incumbent 0 stays, 1 leaves; 4: newcomer 4 at 100, incumbents 0 and 5 tie at 93, position 0
    wins; 5: row 0 is silent and no candidate, incumbent 4 at 93, the newcomers tie at 87 and position 1 wins"""
    P = 6
    sa = np.full((6, P, 1), 200, dtype=np.uint8)
    level = np.full((6, P), 40, dtype=np.uint8)
    level[5, 2] = 34
    level[5, 3] = 33
    level[4, 4] = 27
    sa[0, 5, 0] = 0
    room = np.zeros(6, dtype=np.int32)
    return sa, level, room


TIE_EXPECTED = ([0, 1], [0, 1], [0, 1], [5, 0], [4, 0], [4, 1])       # per packet: the selection in its order (first = dominant)

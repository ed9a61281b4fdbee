"""Inputs and fixture access of the resampler tests (tests/test_resample_model.py, tests/test_gpu_resample.py).

The input rows come from a pure-integer generator written out here (a 32-bit LCG, no library RNG), so the fixture
(tests/golden/resample.npz, written by tests/golden/make_resample.py from the compiled reference) holds expected outputs and states
only, and the inputs are the same everywhere.  Six row families, each PACKETS packets long:

    0  full-scale white noise (the reference saturates on it in every real conversion except 48 -> 8 kHz)
    1  low-level speech-like signal: two slow integer oscillators and a little noise, a few hundred LSB
    2  silence for one packet, then a full-scale step held
    3  a full-scale square wave at fs_in / 6
    4  constant -32768
    5  all zeros (state and output must stay zero)
"""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "resample.npz")

RATES = (8000, 16000, 32000, 48000)
PAIRS = ((48000, 16000), (48000, 32000), (32000, 16000), (16000, 8000), (16000, 32000), (8000, 16000), (16000, 48000), (32000, 48000))
PAIRS_20MS = ((48000, 16000), (16000, 48000))
SATURATING = ((48000, 16000), (48000, 32000), (32000, 16000), (16000, 32000), (16000, 48000), (32000, 48000))
FAMILIES = 6
PACKETS = 4
STATE_BYTES = 96
SEED = 20240611


def lcg(seed, n):
    """n successive values of x -> 1664525 x + 1013904223 (mod 2^32), as Python ints"""
    out, x = [], seed & 0xFFFFFFFF
    for _ in range(n):
        x = (1664525 * x + 1013904223) & 0xFFFFFFFF
        out.append(x)
    return out


def _tri(phase, period, amp):
    """integer triangle wave of the given period (samples) and amplitude"""
    q = phase % period
    h = period // 2
    return (amp * (2 * q - h)) // h if q < h else (amp * (3 * h - 2 * q)) // h


def family_row(family, n, packet, seed=SEED):
    """row of `n` samples (n = PACKETS * packet) of one family -> int16 array"""
    if family == 0:
        v = [(x >> 16) - 32768 for x in lcg(seed + 1, n)]
    elif family == 1:
        r = lcg(seed + 2, n)
        v = [_tri(i, 137, 180) + _tri(3 * i + 11, 59, 90) + ((r[i] >> 20) % 31) - 15 for i in range(n)]
    elif family == 2:
        v = [0 if i < packet else 32767 for i in range(n)]
    elif family == 3:
        v = [32767 if (i // 3) % 2 == 0 else -32768 for i in range(n)]
    elif family == 4:
        v = [-32768] * n
    else:
        v = [0] * n
    a = np.array(v, dtype=np.int64)
    assert a.min() >= -32768 and a.max() <= 32767
    return a.astype(np.int16)


def inputs(fs_in, ms=40, seed=SEED):
    """the six rows at fs_in -> int16 [FAMILIES, PACKETS, packet]"""
    packet = fs_in // 1000 * ms
    return np.stack([family_row(f, PACKETS * packet, packet, seed).reshape(PACKETS, packet) for f in range(FAMILIES)])


def key(fs_in, fs_out, ms=40):
    return "%d_%d_%d" % (fs_in // 1000, fs_out // 1000, ms)


_fixture = None


def fixture():
    global _fixture
    if _fixture is None:
        _fixture = dict(np.load(FIXTURE))
    return _fixture


def expected(fs_in, fs_out, ms=40):
    """(pcm int16 [FAMILIES, packets stored, out packet], state uint8 [FAMILIES, packets stored, 96]) of the fixture"""
    z = fixture()
    k = key(fs_in, fs_out, ms)
    return z["pcm_" + k], z["state_" + k]


def tiled(a, n_rows):
    """row i = family i % 6 of a [FAMILIES, ...] array"""
    return a[np.arange(n_rows) % FAMILIES]

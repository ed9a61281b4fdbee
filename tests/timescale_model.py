"""Independent model of solo_timescale (include/solo_mi355x.h), written from the rules of the interface, not from
solo_amd/csrc/solo_timescale.h: plain numpy arithmetic block by block, all rows of a call at once; and the generator of the input
families the tests run it on."""
import os

import numpy as np

GEOMETRIES = ((16000, 320), (16000, 640), (32000, 640), (32000, 1280))           # (sample rate, packet samples)
FAMILIES = ("speech", "random", "square", "constant", "impulse", "periodic")
PERIODS = (16, 20, 32, 40)
SPEECH_FLOOR = 200                                                                # mean |x| of a speech segment that counts as speech


def geometry(fs, L, a, b):
    H = fs // 200
    return dict(H=H, D=3 * H // 2, Li=a * L, Lo=b * L, M=b * L // H)


def nominal(m, Li, H, M):
    return (2 * m * (Li - H) + (M - 1)) // (2 * (M - 1))


def lag_range(m, Li, H, M):
    """the clipped candidates of a searched block: (first, last)"""
    D, n = 3 * H // 2, nominal(m, Li, H, M)
    return max(-D, -n), min(D, Li - 2 * H - n)


def narrowest_window(cases):
    """fewest candidates of any searched block over (fs, L, a, b) cases"""
    best = None
    for fs, L, a, b in cases:
        g = geometry(fs, L, a, b)
        for m in range(1, g["M"] - 1):
            lo, hi = lag_range(m, g["Li"], g["H"], g["M"])
            best = hi - lo + 1 if best is None else min(best, hi - lo + 1)
    return best


def model_timescale(pcm, out_packets, fs, search=True, lookahead=True):
    """pcm int16 [n, a, L] -> dict(out int16 [n, b, L], shift int32 [n, M], cost int32 [n, M], count, by_abs, by_sign, searched_cost,
    last_cost, first_cost).  search=False pins every lag at the clipped nominal; lookahead=False drops the second term of block M - 2.  by_abs /
    by_sign int [n]: the searched blocks of each row in which several candidates had the least cost and |lag|, respectively the sign,
    decided."""
    n, a, L = pcm.shape
    g = geometry(fs, L, a, out_packets)
    H, Li, Lo, M = g["H"], g["Li"], g["Lo"], g["M"]
    x = pcm.reshape(n, Li).astype(np.int32)                                       # (a cost stays below 2^25)
    y = np.zeros((n, Lo), np.int64)
    shift, cost, first = np.zeros((n, M), np.int64), np.zeros((n, M), np.int64), np.zeros((n, M), np.int64)
    j = np.arange(H)
    rows = np.arange(n)[:, None]
    y[:, :H] = x[:, :H]
    s = np.zeros(n, np.int64)
    by_abs, by_sign = np.zeros(n, np.int64), np.zeros(n, np.int64)
    tail = x[:, Li - H:]
    for m in range(1, M):
        t = x[rows, (s + H)[:, None] + j]                                          # what the previous segment would play next
        if m < M - 1:
            nm = nominal(m, Li, H, M)
            lo, hi = lag_range(m, Li, H, M)
            assert lo <= hi
            d = np.arange(lo, hi + 1)
            if not search:
                d = d[np.argmin(np.abs(d))][None]
            win = np.lib.stride_tricks.sliding_window_view(x[:, nm + lo:nm + hi + 2 * H], H, axis=1)      # [n, lag - lo (and beyond), H]
            c = c1 = np.abs(win[:, d - lo] - t[:, None, :]).sum(axis=2)
            if m == M - 2 and lookahead:
                c = c + np.abs(win[:, d - lo + H] - tail[:, None, :]).sum(axis=2)
            key = (c.astype(np.int64) << 20) + (np.abs(d) << 10) + (d + 512)                        # (cost, |d|, d) in lexicographic order
            k = np.argmin(key, axis=1)
            dm, cm = d[k], c[rows[:, 0], k]
            first[:, m] = c1[rows[:, 0], k]
            least = c == cm[:, None]
            several = least.sum(axis=1) > 1
            least_abs = np.where(least, np.abs(d), 1 << 20).min(axis=1)
            by_abs += several & ((np.abs(d) != least_abs[:, None]) & least).any(axis=1)
            by_sign += (least & (np.abs(d) == least_abs[:, None])).sum(axis=1) > 1
            s = nm + dm
        else:
            s = np.full(n, Li - H, np.int64)
            dm = np.zeros(n, np.int64)
            cm = np.abs(t - tail).sum(axis=1)
        seg = x[rows, s[:, None] + j]
        y[:, m * H:(m + 1) * H] = (t * (H - 1 - j) + seg * (j + 1) + H // 2) // H   # (numpy's // floors)
        shift[:, m], cost[:, m] = dm, cm
    assert y.min() >= -32768 and y.max() <= 32767
    return dict(out=y.astype(np.int16).reshape(n, out_packets, L), shift=shift.astype(np.int32), cost=cost.astype(np.int32),
                count=dict(rows=n, blocks=n * (M - 2), cost=int(cost.sum())), by_abs=by_abs, by_sign=by_sign,
                searched_cost=int(cost[:, 1:M - 1].sum()), first_cost=int(first[:, 1:M - 1].sum()), last_cost=int(cost[:, M - 1].sum()))


_SPEECH = None


def speech():
    """the golden recording (16 kHz, int16)"""
    global _SPEECH
    if _SPEECH is None:
        _SPEECH = np.fromfile(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "Ch_f1_raw.pcm"), dtype="<i2")
    return _SPEECH


def speech_rows(seed, n, length):
    """n segments of the recording with mean |x| >= SPEECH_FLOOR -> int16 [n, length]"""
    sp, rng = speech(), np.random.default_rng(seed)
    rows = []
    while len(rows) < n:
        k = int(rng.integers(0, len(sp) - length))
        seg = sp[k:k + length]
        if np.abs(seg.astype(np.int64)).mean() >= SPEECH_FLOOR:
            rows.append(seg)
    return np.stack(rows)


def speech_segments(length):
    """EVERY segment of the recording, cut back to back from its start, with mean |x| >= SPEECH_FLOOR -> int16 [k, length]"""
    sp = speech()
    segs = sp[:len(sp) // length * length].reshape(-1, length)
    return segs[np.abs(segs.astype(np.int64)).mean(axis=1) >= SPEECH_FLOOR]


def worst_square(fs, L, a, b):
    """a row of +full scale with -full scale from the first candidate of block M - 2 to the start of the last H samples: every candidate
    of that block is 65535 from its template AND from the pinned end in every sample"""
    g = geometry(fs, L, a, b)
    H, Li, M = g["H"], g["Li"], g["M"]
    x = np.full(Li, 32767, np.int16)
    x[nominal(M - 2, Li, H, M) + lag_range(M - 2, Li, H, M)[0]:Li - H] = -32768
    return x


def timescale_rows(seed, n, fs, L, a, b):
    """-> (pcm int16 [n, a, L], family int [n]: index into FAMILIES).  Every family gets n // 6 rows at least (speech the rest):
    random: uniform full scale; square: +-full scale with half periods of 1 .. 4H samples, and worst_square; constant: silence, +-full
    scale and other levels; impulse: one non-zero sample; periodic: a random period of T samples, T in PERIODS and 2 .. 57."""
    rng = np.random.default_rng(seed)
    H, Li = fs // 200, a * L
    q = n // 6
    fam = np.repeat(np.arange(6), [n - 5 * q, q, q, q, q, q])
    x = np.zeros((n, Li), np.int16)
    k = np.arange(Li)
    for i in range(n):
        f, r = FAMILIES[fam[i]], int((fam[:i] == fam[i]).sum())
        if f == "speech":
            x[i] = speech_rows(seed * 1000 + i, 1, Li)[0]
        elif f == "random":
            x[i] = rng.integers(-32768, 32768, Li)
        elif f == "square":
            half = int(rng.integers(1, 4 * H + 1))
            x[i] = worst_square(fs, L, a, b) if r == 0 else np.where(((k + int(rng.integers(0, 2 * half))) // half) & 1, 32767, -32768)
        elif f == "constant":
            x[i] = (0, 32767, -32768, 1, -1)[r] if r < 5 else int(rng.integers(-32768, 32768))
        elif f == "impulse":
            x[i, int(rng.integers(0, Li)) if r else Li - 1] = (32767, -32768)[r & 1]
        else:
            T = PERIODS[r] if r < len(PERIODS) else int(rng.integers(2, 58))
            x[i] = rng.integers(-32768, 32768, T).astype(np.int16)[k % T]
    return x.reshape(n, a, L), fam

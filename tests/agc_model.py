"""Independent model of solo_agc (include/solo_mi355x.h), written from the rule as the header states it and not from the kernel
source: per-row scalars are Python integers, per-sample arrays are numpy int64 (every product of the rule fits: |x g| < 2^37,
|y0 env| < 2^36), all shifts arithmetic.  The tables are built here with `decimal`.  The limiter's envelope is the RECURSION
e_b = min(a'_b, e_{b-1} + release); envelope_closed() is the closed form the kernel uses, for tests/test_agc_model.py to compare."""
from decimal import ROUND_HALF_EVEN, Decimal, getcontext

import numpy as np

import vad_model as VM

STATE_WORDS = 16
INIT = (0, 0, 0, 65536, 32768) + (0,) * 11
PARAMS = ("target", "boost", "cut", "sa_on", "gate", "alpha", "up", "down", "ceiling", "release")
DEFAULTS = dict(target=23, boost=24, cut=12, sa_on=128, gate=50, alpha=32, up=128, down=256, ceiling=29204, release=256)

_tables = None


def tables():
    """A[i] = round(65536 * 10^((i - 30) / 20)), i = 0 .. 60; B[r] = round(65536 * 10^(r / 5120)), r = 0 .. 255"""
    global _tables
    if _tables is None:
        getcontext().prec = 80
        rnd = lambda v: int(v.quantize(Decimal(1), rounding=ROUND_HALF_EVEN))
        A = [rnd(Decimal(65536) * Decimal(10) ** (Decimal(i - 30) / 20)) for i in range(61)]
        B = [rnd(Decimal(65536) * Decimal(10) ** (Decimal(r) / 5120)) for r in range(256)]
        _tables = (A, B)
    return _tables


def lin(d):
    assert -7680 <= d <= 7680
    A, B = tables()
    i, r = divmod(d + 7680, 256)
    return (A[i] * B[r] + 32768) >> 16


def clamp(v, lo, hi):
    return max(lo, min(hi, v))


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    assert sorted(p) == sorted(PARAMS)
    return p


def params_words(**kw):
    p = params(**kw)
    return np.array([p[k] for k in PARAMS], dtype=np.int32)


def attenuations(y0, ceiling):
    """a_b of the blocks of 32 samples of y0 (int64 [L]) -> list"""
    pk = np.abs(y0).reshape(-1, 32).max(axis=1)
    return [32768 if int(v) <= ceiling else (ceiling * 32768) // int(v) for v in pk]


def lookahead(a):
    return [min(a[b], a[b + 1]) for b in range(len(a) - 1)] + [a[-1]]


def envelope(a, env, release):
    """-> [e_{-1}, e_0 .. e_{B-1}] by the recursion"""
    ap = lookahead(a)
    e = [min(env, a[0])]
    for b in range(len(a)):
        e.append(min(ap[b], e[-1] + release))
    return e


def envelope_closed(a, env, release):
    """the same by e_b = min(e_{-1} + (b + 1) rel, min_{j <= b}(a'_j + (b - j) rel))"""
    ap = lookahead(a)
    first = min(env, a[0])
    return [first] + [min(first + (b + 1) * release, min(ap[j] + (b - j) * release for j in range(b + 1))) for b in range(len(a))]


class Agc:
    """state int32 [n_rows, 16]; run() walks the packets of a call"""

    def __init__(self, n_rows):
        self.n_rows = n_rows
        self.state = np.tile(np.array(INIT, dtype=np.int32), (n_rows, 1))

    def state_bytes(self):
        return self.state.view(np.uint8).reshape(self.n_rows, 4 * STATE_WORDS).copy()

    def set_state_bytes(self, blob, rows=None):
        w = np.ascontiguousarray(blob).view(np.int32).reshape(-1, STATE_WORDS)
        for i, r in enumerate(range(len(w)) if rows is None else rows):
            if 0 <= r < self.n_rows:
                self.state[r] = w[i]

    def reset(self, rows=None):
        for r in range(self.n_rows) if rows is None else rows:
            self.state[r] = INIT

    def run(self, pcm, level=None, sa=None, rows=None, **kw):
        """pcm int16 [n, P, L] -> dict(pcm int16 [n, P, L], level uint8 [n, P], gain int16 [n, P], count dict), or None for a refused list
        (nothing moves)"""
        p = params(**kw)
        n, P, L = pcm.shape
        if rows is not None:
            rows = [int(r) for r in rows]
            if len(rows) != n or any(r < 0 or r >= self.n_rows for r in rows) or any(b <= a for a, b in zip(rows, rows[1:])):
                return None
        A, _ = tables()
        out = np.zeros((n, P, L), dtype=np.int16)
        level_out, gain_out = np.zeros((n, P), dtype=np.uint8), np.zeros((n, P), dtype=np.int16)
        n_speech = n_limited = 0
        ramp = np.minimum(np.arange(L, dtype=np.int64) + 1, 256)
        tt = np.tile(np.arange(32, dtype=np.int64) + 1, L // 32)
        for i in range(n):
            st = self.state[i if rows is None else rows[i]]
            run, spl = int(st[0]), int(st[1])
            gain, g, env = clamp(int(st[2]), -7680, 7680), clamp(int(st[3]), 0, A[60]), clamp(int(st[4]), 0, 32768)
            for q in range(P):
                x = pcm[i, q].astype(np.int64)
                # 1. observation
                lv = min(int(level[i, q]), 127) if level is not None else VM.level(pcm[i, q])
                act = 255 if sa is None else int(sa[i, q].max())
                speech = act >= p["sa_on"] and lv <= p["gate"]
                # 2. level and gain
                if speech:
                    n_speech += 1
                    if run == 0:
                        spl, run = lv << 8, 1
                    else:
                        spl += (((lv << 8) - spl) * p["alpha"]) >> 8
                    want = clamp(spl - (p["target"] << 8), -(p["cut"] << 8), p["boost"] << 8)
                    gain += clamp(want - gain, -p["down"], p["up"])
                # 3. gain with a 256-sample ramp
                g0, g1 = g, lin(gain)
                g = g1
                gs = g0 + (((g1 - g0) * ramp) >> 8)
                y0 = (x * gs + 32768) >> 16
                # 4. limiter
                e = envelope(attenuations(y0, p["ceiling"]), env, p["release"])
                env = e[-1]
                n_limited += any(v < 32768 for v in e[1:])
                # 5. output
                e0, e1 = np.repeat(np.array(e[:-1], dtype=np.int64), 32), np.repeat(np.array(e[1:], dtype=np.int64), 32)
                y = (y0 * (e0 + (((e1 - e0) * tt) >> 5)) + 16384) >> 15
                assert int(np.abs(y).max()) <= p["ceiling"]
                out[i, q] = y
                # 6. reports
                level_out[i, q] = VM.level_of_energy(int((y * y).sum()), L)
                gain_out[i, q] = gain
            st[:5] = (run, spl, gain, g, env)
        return dict(pcm=out, level=level_out, gain=gain_out, count=dict(rows=n, speech=n_speech, limited=n_limited, zero=0))

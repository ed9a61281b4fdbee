"""Inputs, generated cases and the host build of the level control tests (tests/test_agc_model.py, tests/test_agc_abi.py,
tests/test_gpu_agc.py).

The PCM rows come from the speech fixture and from a pure-integer generator (the 32-bit LCG of tests/vad_lib.py, no library RNG).  A
case is a list of calls on one object; a call is a dict(pcm int16 [n, P, L], level uint8 [n, P] or None, sa uint8 [n, P, F] or None,
rows list or None, inplace bool, prm dict of parameters that differ from the defaults).  check_case() runs a case through an engine
(the host build here, the C ABI and solo_amd.Agc in the GPU tests) and through tests/agc_model.py, and compares PCM, level_out, gain_q8,
count and the whole state after every call, byte for byte."""
import ctypes as C

import numpy as np

import agc_model as M
from host_build import host_lib
from vad_lib import SEED, speech

STATE_BYTES = 64
SHAPES = [(L, n, P) for L in (320, 640, 1920) for n in (1, 5, 67) for P in (1, 3)]


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def lcg(seed, n):
    """the sequence of vad_lib.lcg (x -> 1664525 x + 1013904223 mod 2^32) as a uint32 array, by doubling: m values and the map of m
    steps (a, c) give the next m values"""
    out = np.empty(n, dtype=np.uint64)
    out[0] = (1664525 * (seed & 0xFFFFFFFF) + 1013904223) & 0xFFFFFFFF
    m, a, c = 1, 1664525, 1013904223
    while m < n:
        k = min(m, n - m)
        out[m:m + k] = (np.uint64(a) * out[:k] + np.uint64(c)) & np.uint64(0xFFFFFFFF)
        a, c, m = (a * a) & 0xFFFFFFFF, (a * c + c) & 0xFFFFFFFF, 2 * m
    return out.astype(np.uint32)


def noise(seed, n, half):
    """sum of four uniform integers of [-half, half] (vad_lib.noise on the sequence above)"""
    r = (lcg(seed, 4 * n).astype(np.int64) >> 16) % (2 * half + 1) - half
    return r.reshape(n, 4).sum(axis=1)


def family_row(seed, k, samples, L):
    """row family k of `samples` samples (packets of L) -> int64 array inside int16"""
    i = np.arange(samples)
    if k == 0:
        return np.resize(speech()[4000:], samples)                              # speech at its own level
    if k == 1:
        return np.clip(noise(seed, samples, 8000) * 2, -32768, 32767)           # loud, peaks far above the ceiling
    if k == 2:
        return np.zeros(samples, dtype=np.int64)
    if k == 3:
        return noise(seed, samples, 12)                                         # level above the gate: no speech
    if k == 4:
        return np.where(i % 32 < 16, 32767, -32768)                             # full scale
    if k == 5:
        x = noise(seed, samples, 300)                                           # peaks at samples 31 and 32 and at L - 1 of its packets
        x[(i % L == 31) & (i // L % 3 == 0)] = 32767
        x[(i % L == 32) & (i // L % 3 == 1)] = -32768
        x[(i % L == L - 1) & (i // L % 3 == 2)] = 32767
        return x
    x = np.resize(speech()[4000:], samples) >> 3                                # quiet speech, wants the whole boost
    x[(i % L >= L - 32) & (i // L % 2 == 0)] = 20000                            # a loud last block, then a louder first block
    x[(i % L < 32) & (i // L % 2 == 1)] = -32768
    return x


N_FAMILIES = 7


def rows_pcm(seed, n, P, L):
    """int16 [n, P, L]: row i of family i % N_FAMILIES"""
    a = np.stack([family_row(seed + 31 * i, i % N_FAMILIES, P * L, L) for i in range(n)])
    assert a.min() >= -32768 and a.max() <= 32767
    return a.astype(np.int16).reshape(n, P, L)


def activities(seed, n, P, F):
    """uint8 [n, P, F]: about a quarter of the packets below the default sa_on_q8 in every frame"""
    r = (lcg(seed, n * P * (F + 1)).astype(np.int64) >> 12).reshape(n, P, F + 1)
    sa = np.where(r[:, :, :1] % 4 == 0, r[:, :, 1:] % 128, 100 + r[:, :, 1:] % 156)
    return sa.astype(np.uint8)


def model_levels(pcm):
    return np.array([[M.VM.level(p) for p in row] for row in pcm], dtype=np.uint8)


def call(pcm, level=None, sa=None, rows=None, inplace=False, **prm):
    return dict(pcm=pcm, level=level, sa=sa, rows=rows, inplace=inplace, prm=prm)


def generated_case(L, n, P, seed=SEED):
    """three calls on an object of n + 3 rows: all defaults with the VAD's inputs; other parameters, no level, no activity, in place; a
    list"""
    a = rows_pcm(seed + L + n, n, 3 * P, L)
    x0, x1, x2 = a[:, :P], a[:, P:2 * P], a[:, 2 * P:]
    F = L // 320 if L % 320 == 0 else 1
    calls = [call(x0, level=model_levels(x0), sa=activities(seed + 7, n, P, F)),
             call(x1, inplace=True, target=20, boost=30, cut=30, alpha=256, up=7680, down=7680, ceiling=12000, release=40),
             call(x2, sa=activities(seed + 8, n, P, 2), rows=[r + (r > 0) + 2 * (r > n // 2) for r in range(n)], up=16, down=8, release=32768)]
    return dict(n_rows=n + 3, calls=calls)


def special_cases(seed=SEED):
    """name -> case: the places where the rule can go wrong, each at the smallest shape that shows it"""
    L = 320
    z = lambda P=1: np.zeros((1, P, L), dtype=np.int16)
    cases = {}
    for name, at in (("peak_31", 31), ("peak_32", 32), ("peak_last", L - 1), ("peak_block0", 5)):
        x = z(2)
        x[0, 0] = noise(seed, L, 200)
        x[0, 0, at] = -32768
        cases[name] = dict(n_rows=1, calls=[call(x, boost=0, cut=0)])
    x = z(2)
    x[0, 0, L - 32:] = 20000
    x[0, 1, :32] = 32767
    cases["louder_next_packet"] = dict(n_rows=1, calls=[call(x, boost=0, cut=0, ceiling=10000)])
    x = z(4)
    x[0, 0, 100] = 32767
    x[0, 1:] = 3000
    cases["slow_release"] = dict(n_rows=1, calls=[call(x[:, :1], boost=0, cut=0, ceiling=8000, release=1000)] +
                                 [call(x[:, p:p + 1], boost=0, cut=0, ceiling=8000, release=1000) for p in (1, 2, 3)])
    x = np.full((1, 2, L), -32768, dtype=np.int16)
    cases["min_sample_max_boost"] = dict(n_rows=1, calls=[call(x, level=np.full((1, 2), 100, dtype=np.uint8), target=0, boost=30, gate=127, alpha=256, up=7680)])
    x = np.tile(rows_pcm(seed, 1, 1, L), (1, 3, 1))
    cases["falling_ramp"] = dict(n_rows=1, calls=[call(x, level=np.array([[60, 5, 5]], dtype=np.uint8), gate=127, alpha=256, up=7680, down=7680, cut=30)])
    cases["zeros"] = dict(n_rows=1, calls=[call(z(2)), call(z(2), level=np.zeros((1, 2), dtype=np.uint8))])
    cases["level_127"] = dict(n_rows=1, calls=[call(rows_pcm(seed, 1, 2, L), level=np.array([[127, 200]], dtype=np.uint8), gate=127)])
    x = rows_pcm(seed, 1, 3, L)
    cases["below_sa_on"] = dict(n_rows=1, calls=[call(x, sa=np.array([[[200, 0], [127, 100], [0, 128]]], dtype=np.uint8), level=np.full((1, 3), 40, dtype=np.uint8))])
    cases["first_speech"] = dict(n_rows=1, calls=[call(x, level=np.array([[90, 30, 31]], dtype=np.uint8))])
    cases["slew_clamps"] = dict(n_rows=1, calls=[call(x, level=np.array([[50, 50, 0]], dtype=np.uint8), up=100, down=7, alpha=256)])
    cases["params_change"] = dict(n_rows=1, calls=[call(x[:, :1]), call(x[:, 1:2], target=10, ceiling=5000, release=0), call(x[:, 2:], target=40, cut=30, down=7680)])
    cases["no_level_in"] = dict(n_rows=1, calls=[call(x)])
    cases["model_level_in"] = dict(n_rows=1, calls=[call(x, level=model_levels(x))])
    cases["no_sa"] = dict(n_rows=1, calls=[call(x, level=model_levels(x))])
    cases["in_place"] = dict(n_rows=2, calls=[call(rows_pcm(seed, 2, 2, L), inplace=True)])
    blob = np.tile(np.array([7, -2000000000, 90000, 1 << 30, -5] + [0x5A5A5A5A] * 11, dtype=np.int32), (3, 1))
    blob[1, :5] = (0, 2000000000, -90000, -1, 1 << 20)
    blob[2, :5] = (-1, 0x7FFFFFFF, 7681, 2072431, 32769)
    cases["blob_out_of_range"] = dict(n_rows=3, blob=blob.view(np.uint8).reshape(3, STATE_BYTES), calls=[call(rows_pcm(seed, 3, 2, L), gate=127)])
    return cases


# ---- the comparison ------------------------------------------------------------------------------------------------------------------------
_reference = {}


def reference(case, tag):
    """the model's run of a case, computed once per tag: (initial state, [(outputs, state after the call)])"""
    if tag not in _reference:
        m = M.Agc(case["n_rows"])
        if "blob" in case:
            m.set_state_bytes(case["blob"])
        first, steps = m.state_bytes(), []
        for c in case["calls"]:
            want = m.run(c["pcm"], level=c["level"], sa=c["sa"], rows=c["rows"], **c["prm"])
            assert want is not None
            steps.append((want, m.state_bytes()))
        _reference[tag] = (first, steps)
    return _reference[tag]


def check_case(engine, case, tag):
    """engine: .run(pcm, level, sa, rows, inplace, **prm) -> dict(pcm, level, gain, count) or None (refused); .state() -> uint8 [n_rows, 64];
    .set_state(blob).  tag: the case's name (the model's run is kept under it)"""
    first, steps = reference(case, tag)
    if "blob" in case:
        engine.set_state(case["blob"])
    assert np.array_equal(engine.state(), first), (tag, "initial state")
    for k, (c, (want, state)) in enumerate(zip(case["calls"], steps)):
        got = engine.run(c["pcm"], c["level"], c["sa"], c["rows"], c["inplace"], **c["prm"])
        assert got is not None, (tag, k)
        for key in ("pcm", "level", "gain"):
            assert np.array_equal(got[key], want[key]), (tag, k, key)
        assert int(np.abs(got["pcm"].astype(np.int32)).max()) <= M.params(**c["prm"])["ceiling"], (tag, k)
        if got["count"] is not None:
            assert got["count"] == want["count"], (tag, k, got["count"], want["count"])
        assert np.array_equal(engine.state(), state), (tag, k, "state")


# ---- the host build of solo_agc.h ------------------------------------------------------------------------------------------------------------
def build_host():
    lib, V, I = host_lib("agc"), C.c_void_p, C.c_int
    lib.emu_agc_init.argtypes = [V, I]
    lib.emu_agc_prefix_min_steps.argtypes = [V]
    lib.emu_agc_list_ok.argtypes = [V, I, I]
    lib.emu_agc_call_ok.argtypes = [I, V, I, V, I, I, V, I, V, V, V]
    lib.emu_agc_run.argtypes = [I, V, V, I, V, I, I, V, V, I, V, V, V, V, V]
    return lib


def _p(a):
    return None if a is None else a.ctypes.data


class HostEngine:
    def __init__(self, lib, n_rows):
        self.lib, self.n_rows = lib, n_rows
        self.st = np.zeros((n_rows, 16), dtype=np.int32)
        lib.emu_agc_init(_p(self.st), n_rows)
        self.status = 0

    def state(self):
        return self.st.view(np.uint8).reshape(self.n_rows, STATE_BYTES).copy()

    def set_state(self, blob):
        self.st[:len(blob)] = np.ascontiguousarray(blob).view(np.int32).reshape(-1, 16)

    def run(self, pcm, level, sa, rows, inplace, count=True, **prm):
        n, P, L = pcm.shape
        buf = np.zeros(pcm.size + 8, dtype=np.int16)                            # a 16-byte aligned copy
        off = (-buf.ctypes.data % 16) // 2
        x = buf[off:off + pcm.size].reshape(pcm.shape)
        x[...] = pcm
        obuf = np.full(pcm.size + 8, 0x5A5A, dtype=np.int16)
        ooff = (-obuf.ctypes.data % 16) // 2
        out = x if inplace else obuf[ooff:ooff + pcm.size].reshape(pcm.shape)
        level = None if level is None else np.ascontiguousarray(level, dtype=np.uint8)
        sa = None if sa is None else np.ascontiguousarray(sa, dtype=np.uint8)
        rows_a = None if rows is None else np.array(rows, dtype=np.int32)
        lo, go = np.full((n, P), 0x5A, dtype=np.uint8), np.full((n, P), 0x5A5A, dtype=np.int16)
        cnt = np.full(4, 0x5A5A, dtype=np.int32)
        w = M.params_words(**prm)
        self.status = self.lib.emu_agc_run(self.n_rows, _p(self.st), _p(rows_a), n, _p(x), P, L, _p(level), _p(sa), 0 if sa is None else sa.shape[2], _p(w),
                                           _p(out), _p(lo), _p(go), _p(cnt) if count or rows is not None else None)
        self.raw = dict(pcm=out.copy(), level=lo, gain=go, count=cnt)
        if self.status:
            return None
        return dict(pcm=out.copy(), level=lo, gain=go, count=dict(zip(("rows", "speech", "limited", "zero"), (int(v) for v in cnt))) if count or rows is not None else None)

"""solo_rate on the CPU: the host build of solo_amd/csrc/solo_rate.h (tests/rate_host.cpp) against tests/rate_model.py word for word --
state, both outputs and counts over the constructed feedback sequences --, the send mask rule, and sx_enc_setup_rate driven by a value of
solo_batch_update_rates.  From the model alone: the sequences reach every place of the rule."""
import ctypes as C

import numpy as np
import pytest

import rate_model as M
from host_build import host_lib


@pytest.fixture(scope="module")
def host():
    return host_lib("rate")


class HostRate:
    """the object as the host build sees it: the caller carries the state"""

    def __init__(self, lib, n_rows):
        self.lib, self.n_rows = lib, n_rows
        self.st = np.full((n_rows, M.WORDS), 0x5A5A5A5A, dtype=np.int32)
        lib.emu_rate_init(self.st.ctypes.data, n_rows)

    def update(self, feedback, p):
        fb = np.zeros(self.n_rows * 8 + 4, dtype=np.int32)
        off = (-fb.ctypes.data % 16) // 4                   # (the call wants d_feedback on 16 bytes)
        fb[off:off + self.n_rows * 8] = feedback.reshape(-1)
        target = np.full(self.n_rows, -7, dtype=np.int32)
        mode = np.full(self.n_rows, 9, dtype=np.uint8)
        count = np.full(16, -1, dtype=np.int32)
        prm = M.params_words(p)
        r = self.lib.emu_rate_update(self.n_rows, self.st.ctypes.data, fb.ctypes.data + 4 * off, prm.ctypes.data, target.ctypes.data, mode.ctypes.data,
                                     count.ctypes.data)
        assert r == 0
        assert not count[len(M.COUNT):].any()
        return target, mode, dict(zip(M.COUNT, (int(v) for v in count)))


def _same(host_out, model_out, where):
    for a, b, name in zip(host_out, model_out, ("target", "mode", "count")):
        assert (a == b) if isinstance(a, dict) else np.array_equal(a, b), (where, name, a, b)


@pytest.mark.parametrize("n_rows", [1, 8, 67])
def test_sequences_host_equals_model(host, n_rows):
    h, m = HostRate(host, n_rows), M.Rate(n_rows)
    for c in range(M.CALLS):
        fb = M.feedback(n_rows, c)
        _same(h.update(fb, M.TEST_PARAMS), m.update(fb, M.TEST_PARAMS), c)
        assert np.array_equal(h.st, m.state()), c
        if c == 17 and n_rows > 2:                          # a listed reset in the middle of a run
            rows = list(range(1, n_rows, 3))
            m.reset(rows)
            for r in rows:
                host.emu_rate_init(h.st[r:].ctypes.data, 1)
    assert np.array_equal(h.st[:, M.LIVE:], np.zeros((n_rows, M.WORDS - M.LIVE), dtype=np.int32))


def test_other_parameters_and_foreign_state(host):
    """the binding's defaults, thinning off, a quantum of 1, the widest rates; and records nobody's step wrote: a total rule"""
    n = 64
    sets = [M.params(6000, 40000, 16000), M.params(5000, 1000000, 5000, quantum_bps=1, inc_q8=256, lo_q8=0, hi_q8=0, stale_calls=0),
            M.params(8000, 8000, 8000, quantum_bps=8000, thin_after=1, thin_release=0), M.params(1, 1000000, 500000, quantum_bps=1, lo_q8=255, hi_q8=255, inc_q8=0)]
    for k, p in enumerate(sets):
        assert M.params_ok(p)
        h, m = HostRate(host, n), M.Rate(n)
        if k % 2:
            rng = np.random.default_rng(90 + k)
            words = rng.integers(-2 ** 31, 2 ** 31, size=(n, M.WORDS), dtype=np.int64).astype(np.int32)
            words[::3, 0] &= 7
            h.st[:] = words
            m.set_state(words)
        for c in range(M.CALLS):
            fb = M.feedback(n, c)
            _same(h.update(fb, p), m.update(fb, p), (k, c))
            assert np.array_equal(h.st, m.state()), (k, c)


def test_the_sequences_reach_every_branch():
    """from the model alone"""
    n = 4 * M.N_FAMILIES
    m = M.Rate(n)
    total = dict.fromkeys(M.COUNT, 0)
    targets = set()
    for c in range(M.CALLS):
        t, mode, count = m.update(M.feedback(n, c), M.TEST_PARAMS)
        for k, v in count.items():
            total[k] += v
        targets |= set(int(v) for v in t)
        if c == 0:
            assert count["started"] == count["changed"] == n and (t > 0).all()
    missing = M.REQUIRED_HITS - m.hits
    assert not missing, missing
    assert all(total[k] > 0 for k in M.COUNT), total
    p = M.TEST_PARAMS
    assert p["min_bps"] in targets and p["max_bps"] in targets and 0 in targets
    # the stale step comes in the call in which idle reaches stale_calls, once: family 4 is silent from call 6 on (two repeated blocks first)
    w = list(M.INIT)
    stale_at = [c for c in range(M.CALLS) if "stale" in M.step(w, p, *M.family(4, 0, c))[2]]
    assert stale_at == [6 + p["stale_calls"] - 1]
    # thinning: on after thin_after reports at the floor, an increase refused while thin, off after thin_release clean reports
    w, log = list(M.INIT), []
    for c in range(M.CALLS):
        log.append(M.step(w, p, *M.family(1, 0, c)))
    on = [c for c, (_, _, ev) in enumerate(log) if "thin_on" in ev]
    off = [c for c, (_, _, ev) in enumerate(log) if "thin_off" in ev]
    assert len(on) == 1 and off == [8 + p["thin_release"] - 1] and on[0] < 8
    assert all(log[c][1] == 1 for c in range(on[0], off[0])) and log[off[0]][1] == 0 and "increased" in log[off[0] + 1][2]
    assert "held" in log[8][2] and "increased" not in log[8][2]
    # the wrap: family 5 crosses 2^32 and every advancing block is used
    w = list(M.INIT)
    evs = [M.step(w, p, *M.family(5, 0, c))[2] for c in range(M.CALLS)]
    assert M.family(5, 0, 6)[2] > M.family(5, 0, 7)[2] and all("used" in e for c, e in enumerate(evs) if c != 12) and "repeated" in evs[12]


def test_params_rule(host):
    ok = lambda p: host.emu_rate_params_ok(M.params_words(p).ctypes.data)
    good = M.params(6000, 40000, 16000)
    assert ok(good) == 1 and M.params_ok(good)
    bad = [dict(min_bps=40200), dict(start_bps=5800), dict(start_bps=40200), dict(quantum_bps=0), dict(quantum_bps=-200), dict(min_bps=6100),
           dict(max_bps=40100), dict(start_bps=16100), dict(max_bps=1000200), dict(min_bps=0, quantum_bps=1), dict(min_bps=-200), dict(lo_q8=-1),
           dict(lo_q8=27), dict(hi_q8=256), dict(inc_q8=-1), dict(inc_q8=257), dict(rtt_guard=-1), dict(stale_calls=-1), dict(thin_after=-1),
           dict(thin_release=-1), dict(reserved=1), dict(reserved=-1)]
    for kw in bad:
        p = dict(good, **kw)
        assert ok(p) == 0 and not M.params_ok(p), kw
    edge = [dict(min_bps=1, max_bps=1000000, start_bps=1, quantum_bps=1), dict(lo_q8=0, hi_q8=0), dict(lo_q8=255, hi_q8=255), dict(inc_q8=0),
            dict(inc_q8=256), dict(min_bps=16000, max_bps=16000), dict(rtt_guard=2 ** 31 - 1, stale_calls=2 ** 31 - 1, thin_after=2 ** 31 - 1)]
    for kw in edge:
        p = dict(good, **kw)
        assert ok(p) == 1 and M.params_ok(p), kw
    assert host.emu_rate_params_ok(None) == 0


def _host_mask(host, mode, P, streams=None, seq_base=None, first_seq=0, send_in=None, inplace=False, n=None):
    mode = np.asarray(mode, dtype=np.uint8)
    n = (len(mode) if n is None else n) if streams is None else len(streams)
    lst = None if streams is None else np.asarray(streams, dtype=np.int32)
    base = None if seq_base is None else np.asarray(seq_base, dtype=np.int32)
    sin = None if send_in is None else np.ascontiguousarray(send_in, dtype=np.uint8)
    out = sin if inplace else np.full((n, P), 0xEE, dtype=np.uint8)
    before = out.copy()
    ptr = lambda a: None if a is None else a.ctypes.data
    r = host.emu_rate_send_mask(mode.ctypes.data, len(mode), ptr(lst), n, P, ptr(base), first_seq, ptr(sin), out.ctypes.data)
    if r == -2:
        assert np.array_equal(out, before)
        return None
    assert r == 0
    return out


def test_mask_rule(host):
    assert [M.mask(0, s) for s in (0, 1)] == [3, 3] and [M.mask(1, s) for s in (0, 1, 2, 0xFFFFFFFF)] == [1, 2, 1, 2]
    mode = [0, 1, 1, 0, 1, 1, 0]
    rng = np.random.default_rng(5)
    for first in (0, 1, 7, 10, -1, -2 ** 31, 2 ** 31 - 1):      # odd and even first_seq, and the ends of int32
        for base in (None, [0, -1, -2, 5, 2 ** 31 - 1, -2 ** 31, 3]):
            for P in (1, 4):
                sin = rng.integers(0, 4, size=(len(mode), P)).astype(np.uint8)
                want = M.send_mask(mode, P, seq_base=base, first_seq=first)
                assert np.array_equal(_host_mask(host, mode, P, seq_base=base, first_seq=first), want)
                # a thin row alternates from packet to packet, the parity set by first_seq + seq_base
                for i, mo in enumerate(mode):
                    par = (first + (base[i] if base else 0)) & 1
                    assert list(want[i]) == ([3] * P if not mo else [(2 if (par + k) & 1 else 1) for k in range(P)])
                masked = M.send_mask(mode, P, seq_base=base, first_seq=first, send_in=sin)
                assert np.array_equal(masked, want & sin)
                assert np.array_equal(_host_mask(host, mode, P, seq_base=base, first_seq=first, send_in=sin), masked)
                assert np.array_equal(_host_mask(host, mode, P, seq_base=base, first_seq=first, send_in=sin.copy(), inplace=True), masked)
    # lists: a subset; one that is not increasing, twice the same, out of range: nothing written
    lst, base = [1, 3, 4], [-3, 0, 8]
    want = M.send_mask(mode, 3, streams=lst, seq_base=base, first_seq=5)
    assert list(want[0]) == [1, 2, 1] and list(want[1]) == [3, 3, 3] and list(want[2]) == [2, 1, 2]
    assert np.array_equal(_host_mask(host, mode, 3, streams=lst, seq_base=base, first_seq=5), want)
    for bad in ([3, 1, 4], [1, 1, 4], [1, 3, 7], [-1, 3, 4]):
        assert M.send_mask(mode, 3, streams=bad) is None and _host_mask(host, mode, 3, streams=bad) is None
    # fewer positions than rows without a list
    assert np.array_equal(_host_mask(host, mode, 2, n=3), M.send_mask(mode, 2, n=3))


def test_setup_rate_under_a_target_value(host):
    """a positive value is the targetRate_bps of solo_batch_update_streams: minus 1600 (800 joint), clamped to [5000, 100000], then
    setup_rate on the two SNR words and nothing else; <= 0 and a refused value leave every byte"""
    size = host.emu_rate_enc_state_bytes()
    snr = sorted(host.emu_rate_snr_offset(k) for k in (0, 1))
    assert snr[1] == snr[0] + 4
    fresh = lambda: np.frombuffer(bytes((37 * k + 11) & 0xFF for k in range(size)), dtype=np.uint8).copy()
    I32_MAX = 2 ** 31 - 1
    knots = (8000, 9000, 11000, 13000, 16000, 22000, 11000, 14000, 17000, 21000, 26000, 36000)
    values = [0, -1, -2 ** 31, 1, 799, 800, 801, 1599, 1600, 1601, 5799, 5800, 5801, 6599, 6600, 6601, 100800, 100801, 101600, 101601, 150000, I32_MAX]
    values += [off + m * k + d for off in (800, 1600) for k in knots for m in (1, 2) for d in (-1, 0, 1)] + [14799, 14800, 15599, 15600]
    seen = set()
    for joint in (0, 1):
        for wb in (0, 1):
            for v in values:
                kind, silk = M.apply_target(v, bool(joint), bool(wb))
                seen.add(kind)
                a, b = fresh(), fresh()
                r = host.emu_rate_apply_target(a.ctypes.data, v, joint, 14000 if wb else 0)
                assert r == {"kept": 0, "applied": 1, "refused": 2}[kind], (v, joint, wb)
                if kind == "applied":
                    assert 5000 <= silk <= 100000
                    host.emu_rate_setup_rate(b.ctypes.data, v - (800 if joint else 1600))          # what update_streams hands to the kernel
                    c = fresh()
                    host.emu_rate_setup_rate(c.ctypes.data, silk)                                  # ... and the clamp is setup_rate's own
                    assert np.array_equal(b, c)
                assert np.array_equal(a, b), (v, joint, wb)
                keep = np.ones(size, dtype=bool)
                keep[snr[0]:snr[0] + 8] = False
                assert np.array_equal(a[keep], fresh()[keep])
    assert seen == {"kept", "applied", "refused"}
    assert M.apply_target(15599, False, True)[0] == "refused" and M.apply_target(15600, False, True) == ("applied", 14000)
    assert M.apply_target(14799, True, True)[0] == "refused" and M.apply_target(14800, True, True) == ("applied", 14000)
    assert M.apply_target(1, False, False) == ("applied", 5000) and M.apply_target(I32_MAX, True, False) == ("applied", 100000)


def _argtypes(lib):
    lib.emu_rate_update.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.emu_rate_send_mask.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.emu_rate_init.argtypes = [C.c_void_p, C.c_int]
    lib.emu_rate_params_ok.argtypes = [C.c_void_p]
    lib.emu_rate_apply_target.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    lib.emu_rate_setup_rate.argtypes = [C.c_void_p, C.c_int]


@pytest.fixture(scope="module", autouse=True)
def _declare(host):
    _argtypes(host)

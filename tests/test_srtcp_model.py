"""The SRTCP stage (solo_srtcp_protect / solo_srtcp_unprotect, solo_rtcp_set_trailer; solo_amd/csrc/solo_srtcp.h) without a GPU: the
per-datagram functions, the host forms and the control plane are compiled for the host by this test (tests/srtcp_host.cpp, through
tests/host_build.py) and compared byte for byte with the independent model of tests/srtcp_model.py, whose session keys are checked
against the openssl command-line tool.  Then build's trailer, the control plane's refusals, the ABI, the binding's checks, the built
library's new kernels (no scratch), and the hostile family once more through a stand-alone build of the same source under the address
and undefined-behaviour sanitisers."""
import ast
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import rtcp_model as R
import solo_testlib as T
import srtcp_model as M
from host_build import FLAGS, host_lib, source

SRTCP_SYMBOLS = {"solo_rtcp_set_trailer": 2, "solo_srtcp_set_keys": 8, "solo_srtcp_clear_keys": 4, "solo_srtcp_get_index": 6, "solo_srtcp_protect": 10,
                 "solo_srtcp_unprotect": 8}
KERNELS = ("solo_srtcp_protect_kernel", "solo_srtcp_unprotect_kernel", "solo_srtcp_rx_fold_kernel")
FILL8, FILL32 = 0xA5, -7
L = 640
NOW = 0x83AA7E8000000000
VP, I, LL, U64 = C.c_void_p, C.c_int, C.c_longlong, C.c_uint64


@pytest.fixture(scope="module")
def host():
    lib = host_lib("srtcp")
    lib.emu_rtcp_create.restype = VP
    lib.emu_rtcp_create.argtypes = [I]
    lib.emu_rtcp_destroy.argtypes = [VP]
    lib.emu_rtcp_state.argtypes = [VP, VP, I]
    lib.emu_rtcp_set_cname.argtypes = [VP, VP, I, VP]
    lib.emu_rtcp_table.argtypes = [VP, I, VP]
    lib.emu_rtcp_build.argtypes = [VP, VP, I, I, VP, I, VP, I, U64, VP, VP, VP, LL, VP]
    lib.emu_rtcp_parse.argtypes = [VP, VP, I, VP, I, VP, I, VP, LL, U64, VP, VP, VP]
    lib.emu_srtcp_create.restype = VP
    lib.emu_srtcp_create.argtypes = [VP, I]
    lib.emu_srtcp_destroy.argtypes = [VP]
    lib.emu_srtcp_unbind.argtypes = [VP, VP, I]
    lib.emu_srtcp_set_keys.argtypes = [VP, VP, I, VP, VP, VP, VP]
    lib.emu_srtcp_clear_keys.argtypes = [VP, VP, I]
    lib.emu_srtcp_get_index.argtypes = [VP, VP, I, VP, VP]
    lib.emu_srtcp_snapshot.argtypes = [VP, VP]
    lib.emu_srtcp_key_words.argtypes = [VP, I]
    lib.emu_srtcp_derive.argtypes = [VP] * 5
    lib.emu_srtcp_build.argtypes = [VP, VP, I, I, VP, I, VP, I, U64, VP, VP, LL, VP, I]
    lib.emu_srtcp_protect.argtypes = [VP, I, I, VP, I, VP, VP, VP, LL, VP]
    lib.emu_srtcp_unprotect.argtypes = [VP, VP, I, VP, LL, VP, VP]
    return lib


def p(x):
    return None if x is None else x.ctypes.data


def count_dict(cnt):
    return dict(zip(M.VERDICTS, (int(v) for v in cnt)))


def build_count_of(a):
    return dict(built=int(a[0]), built_needed=int(a[1]), bytes=int(a[2:4].view(np.int64)[0]), bytes_needed=int(a[4:6].view(np.int64)[0]),
                refused=int(a[6]), with_sr=int(a[7]))


def aligned_bytes(n, fill=FILL8):
    """uint8 [n] at a 4-byte aligned address"""
    backing = np.full(n + 8, fill, np.uint8)
    a0 = (-backing.ctypes.data) % 4
    return backing[a0:a0 + n]


class HostRtcp:
    """the RTCP object of the host build, with build's trailer switch"""

    def __init__(self, lib, n):
        self.lib, self.n, self.trailer = lib, n, 0
        self.h = lib.emu_rtcp_create(n)

    def words(self):
        w = np.zeros((self.n, 40), np.uint32)
        self.lib.emu_rtcp_state(self.h, p(w), 0)
        return w

    def set_words(self, w):
        w = np.ascontiguousarray(w, np.uint32)
        self.lib.emu_rtcp_state(self.h, p(w), 1)

    def build(self, tx, rx, streams, now, cap, room=None, guard=64, plain=False):
        """-> (r, dgrams, wire [room + guard], count array int32 [8] (8-byte aligned), count dict); plain: the call without the switch"""
        idx = np.asarray(streams, np.int32)
        room = int(min(cap, 112 * len(idx))) if room is None else room
        dg, wire = np.full((len(idx) + 2, 2), FILL32, np.int32), aligned_bytes(room + guard)
        cnt = np.full(6, -1, np.int64).view(np.int32)
        ctx, crx = tx.cfg(), None if rx is None else rx.cfg()
        if plain:
            r = self.lib.emu_rtcp_build(self.h, p(ctx), tx.n, tx.L, p(crx), 0 if rx is None else rx.n, p(idx), len(idx), now, None, p(dg), p(wire), cap, p(cnt))
        else:
            r = self.lib.emu_srtcp_build(self.h, p(ctx), tx.n, tx.L, p(crx), 0 if rx is None else rx.n, p(idx), len(idx), now, p(dg), p(wire), cap, p(cnt), self.trailer)
        assert (cnt[8:] == -1).all() and (dg[len(idx):] == FILL32).all() and (wire[min(cap, room):] == FILL8).all()
        if r == 1:
            assert (dg == FILL32).all() and (wire == FILL8).all() and (cnt[1:] == -1).all() and cnt[0] == -1
            return r, dg[:len(idx)], wire, cnt, dict(built=-1)
        c = build_count_of(cnt)
        assert (wire[c["bytes"]:] == FILL8).all()            # nothing at or beyond what was written, the cap included
        return r, dg[:len(idx)], wire, cnt, c

    def parse(self, rx, tx, dgrams, wire, now):
        fb, cnt = np.full((self.n + 1, 8), 0xA5A5A5A5, np.uint32), np.full(16 + 4, FILL32, np.int32)
        trx, ttx = np.zeros(4 + 2 * rx.n, np.uint32), np.zeros(4 + 2 * tx.n, np.uint32)
        assert self.lib.emu_rtcp_table(p(rx.cfg()), rx.n, p(trx)) == 0 and self.lib.emu_rtcp_table(p(tx.cfg()), tx.n, p(ttx)) == 0
        wire, dgrams = np.ascontiguousarray(wire), np.ascontiguousarray(dgrams, np.int32)
        assert self.lib.emu_rtcp_parse(self.h, p(trx), rx.n, p(ttx), tx.n, p(dgrams), dgrams.shape[0], p(wire), wire.shape[0], now, None, p(fb), p(cnt)) == 0
        return fb[:self.n].copy(), dict(zip(R.PARSE_COUNT, (int(v) for v in cnt)))

    def close(self):
        self.lib.emu_rtcp_destroy(self.h)


class HostSes:
    """the host form's session: the records of an rtcp_model.Session, keyed as the test says"""

    def __init__(self, lib, session, keys=None, tx_state=None, rx_state=None):
        self.lib, self.n = lib, session.n
        self.h = lib.emu_srtcp_create(p(session.cfg()), session.n)
        assert self.h
        for d in ("tx", "rx"):
            ss = sorted(s for s, k in (keys or {}).items() if k.get(d) is not None)
            if ss:
                kw = dict(tx_index=[(tx_state or {}).get(s, 0) for s in ss]) if d == "tx" else dict(rx_index=[(rx_state or {}).get(s, -1) for s in ss])
                assert self.set_keys(ss, **{d: [keys[s][d] for s in ss]}, **kw) == 0

    def set_keys(self, streams, tx=None, rx=None, tx_index=None, rx_index=None):
        s = np.array(streams, np.int32)
        txa = None if tx is None else np.frombuffer(b"".join(tx), np.uint8)
        rxa = None if rx is None else np.frombuffer(b"".join(rx), np.uint8)
        ti = None if tx_index is None else np.array(tx_index, np.uint32)
        ri = None if rx_index is None else np.array(rx_index, np.int64)
        return self.lib.emu_srtcp_set_keys(self.h, p(s), len(streams), p(txa), p(rxa), p(ti), p(ri))

    def clear_keys(self, streams):
        s = np.array(streams, np.int32)
        return self.lib.emu_srtcp_clear_keys(self.h, p(s), len(streams))

    def unbind(self, streams):
        s = np.array(streams, np.int32)
        return self.lib.emu_srtcp_unbind(self.h, p(s), len(streams))

    def index(self, streams=None):
        s = np.array(range(self.n) if streams is None else streams, np.int32)
        tx, rx = np.full(s.size, 77, np.uint32), np.full(s.size, -5, np.int64)
        assert self.lib.emu_srtcp_get_index(self.h, p(s), s.size, p(tx), p(rx)) == 0
        return tx.tolist(), rx.tolist()

    def snapshot(self):
        out = np.zeros(self.lib.emu_srtcp_snapshot(self.h, None), np.uint8)
        self.lib.emu_srtcp_snapshot(self.h, p(out))
        return out.tobytes()

    def protect(self, streams, build_cnt, dg, wire, wire_bytes=None, trailer=14, rtcp_streams=None):
        s = np.asarray(streams, np.int32)
        cnt = np.full(8 + 4, -9, np.int32)
        r = self.lib.emu_srtcp_protect(self.h, self.n if rtcp_streams is None else rtcp_streams, trailer, p(s), s.size, p(build_cnt), p(dg), p(wire),
                                       wire.size if wire_bytes is None else wire_bytes, p(cnt))
        assert (cnt[8:] == -9).all()
        return r, count_dict(cnt[:8])

    def unprotect(self, dg, wire, wire_bytes=None):
        dg = np.ascontiguousarray(dg, np.int32).reshape(-1, 2)
        out, cnt = np.full((dg.shape[0] + 4, 2), FILL32, np.int32), np.full(8 + 4, -9, np.int32)
        assert self.lib.emu_srtcp_unprotect(self.h, p(dg), dg.shape[0], p(wire), wire.size if wire_bytes is None else wire_bytes, p(out), p(cnt)) == 0
        assert (out[dg.shape[0]:] == FILL32).all() and (cnt[8:] == -9).all()
        return out[:dg.shape[0]], count_dict(cnt[:8])

    def close(self):
        self.lib.emu_srtcp_destroy(self.h)


def sessions(n):
    """X (our streams) and Y (the peers'): SSRCs in no order"""
    X = R.Session([0x10000000 + (s * 2654435761) % 0xFFFFF for s in range(n)], [(0xFFFFF000 + 977 * s) & R.M32 for s in range(n)], packet_samples=L)
    Y = R.Session([0xE0000000 - 31 * s * s - s for s in range(n)], [12345 * s for s in range(n)], packet_samples=L)
    return X, Y


def fill_state(rng, model, shapes=None):
    """rows with something to report; shapes: {stream: (sr, rb, name length)}, the others at random -- every row has received and has a CNAME"""
    for s, r in enumerate(model.rows):
        sr, rb, nl = (shapes or {}).get(s, (int(rng.integers(0, 2)), int(rng.integers(0, 2)), int(rng.integers(1, 32))))
        r.update(base_seq=int(rng.integers(0, 65536)), max_seq=int(rng.integers(0, 65536)), cycles=65536 * int(rng.integers(0, 3)), bad_seq=65537,
                 received=int(rng.integers(1, 5000)), expected_prior=int(rng.integers(0, 100)), received_prior=int(rng.integers(0, 100)),
                 transit=int(rng.integers(0, 2 ** 32)), jitter=int(rng.integers(0, 4000)), seen=(3 if rb else 0) | (4 if rng.integers(0, 2) else 0),
                 lsr=int(rng.integers(0, 2 ** 32)), lsr_arrival=int(rng.integers(0, 2 ** 32)), tx_packets=int(rng.integers(0, 9000)),
                 tx_octets=int(rng.integers(0, 2 ** 32)), tx_next=int(rng.integers(0, 9000)), tx_since=int(rng.integers(1, 50)) if sr else 0)
        model.cname[s] = bytes(rng.integers(97, 123, nl, dtype=np.uint8))
    return model


def pair(host, rng, n, shapes=None):
    """an RTCP object of the host build and its model in the same state"""
    model = fill_state(rng, R.Model(n), shapes)
    h = HostRtcp(host, n)
    h.set_words(model.words())
    return h, model


def both_build(h, model, tx, rx, streams, now, cap, trailer, room=None):
    """build with the trailer on both sides, compared -> (dgrams, wire, count array, model's count)"""
    h.trailer = trailer
    r, dg, wire, cnt, c = h.build(tx, rx, streams, now, cap, room)
    refused, mdg, mwire, mc = M.model_build_trailer(model, tx, rx, list(streams), now, cap, trailer)
    assert (r == 1) == refused
    if refused:
        return dg, wire, cnt, mc
    assert c == mc, (c, mc)
    assert dg.tolist() == [list(d) for d in mdg]
    assert wire[:len(mwire)].tobytes() == mwire and np.array_equal(h.words(), model.words())
    return dg, wire, cnt, mc


# ---- the model's session keys against another implementation ---------------------------------------------------------------------------------
B3_KEY, B3_SALT = bytes.fromhex("E1F97A0D3E018BE0D64FA32C06DE4139"), bytes.fromhex("0EC675AD498AFEEBB6960B3AABE6")


@pytest.mark.skipif(shutil.which("openssl") is None, reason="no openssl command-line tool on this box")
def test_model_session_keys_against_openssl():
    """RFC 3711 publishes no vector for labels 3 .. 5: AES-128-ECB of the counter blocks under the B.3 master key, by openssl"""
    k = M.session_keys(B3_KEY + B3_SALT)
    for label, name, n in ((3, "ke", 16), (4, "ka", 20), (5, "ks", 14)):
        iv = (int.from_bytes(B3_SALT, "big") ^ (label << 48)) << 16
        blocks = b"".join((iv + j).to_bytes(16, "big") for j in range((n + 15) // 16))
        r = subprocess.run(["openssl", "enc", "-aes-128-ecb", "-nopad", "-K", B3_KEY.hex()], input=blocks, capture_output=True)
        assert r.returncode == 0, r.stderr
        assert r.stdout[:n] == k[name], (label, r.stdout.hex(), k[name].hex())
    assert len({k["ke"], k["ka"][:16], k["ks"]}) == 3


def test_host_derivation_equals_the_model(host):
    rng = np.random.default_rng(1)
    for master in (B3_KEY + B3_SALT, rng.integers(0, 256, 30, dtype=np.uint8).tobytes()):
        ke, ks, ka, rec = np.zeros(16, np.uint8), np.zeros(14, np.uint8), np.zeros(20, np.uint8), np.zeros(64, np.uint32)
        host.emu_srtcp_derive(master, p(ke), p(ks), p(ka), p(rec))
        k = M.session_keys(master)
        assert (ke.tobytes(), ks.tobytes(), ka.tobytes()) == (k["ke"], k["ks"], k["ka"])
        assert rec[58] == 10 and rec[59] == 1                       # SxSrtpKey as it is: tag = 10, has
        assert M.session_keys(master) != __import__("srtp_model").session_keys(master)


# ---- build with a trailer ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trailer", [0, 14, 16, 1])
def test_build_with_a_trailer(host, trailer):
    n = 40
    X, Y = sessions(n)
    X.bound[7] = 0
    streams = [s for s in range(n) if s != 20]
    h, model = pair(host, np.random.default_rng(3), n)
    model.cname[11] = b""
    h.set_words(model.words())
    start = model.words().copy()
    dg, wire, cnt, c = both_build(h, model, X, Y, streams, NOW, 2 ** 40, trailer)
    assert c["refused"] == 2 and c["built"] == len(streams) - 2
    gaps = [int(b[0]) - int(a[0]) - int(a[1]) for a, b in zip([d for d in dg.tolist() if d[1]], [d for d in dg.tolist() if d[1]][1:])]
    assert all(trailer <= g < trailer + 4 for g in gaps) and all(d[0] % 4 == 0 and d[1] % 4 == 0 for d in dg.tolist())
    for off, ln in dg.tolist():
        if ln:
            assert not wire[off + ln:off + ((ln + trailer + 3) & ~3)].any()
    if trailer == 0:                                                  # every byte, count and state word as without the call
        h2 = HostRtcp(host, n)
        h2.set_words(start)
        r, dg2, wire2, cnt2, c2 = h2.build(X, Y, streams, NOW, 2 ** 40, plain=True)
        assert np.array_equal(dg, dg2) and np.array_equal(wire, wire2) and np.array_equal(cnt, cnt2) and np.array_equal(h.words(), h2.words())
        h2.close()
    # caps one byte either side of a packet's trailer end, and of its own end
    k = 17
    ends = [int(dg[k][0]) + ((int(dg[k][1]) + trailer + 3) & ~3), int(dg[k][0]) + int(dg[k][1])]
    for cap in sorted({e + d for e in ends for d in (-1, 0, 1)}):
        h.set_words(start)
        model.set_words(start)
        dgc, _, _, cc = both_build(h, model, X, Y, streams, NOW, cap, trailer, room=cap)
        assert (dgc[k][1] != 0) == (cap >= ends[0]) and cc["bytes_needed"] == c["bytes_needed"]
    h.close()


# ---- protect -----------------------------------------------------------------------------------------------------------------------------------
PROTECT_SHAPES = {0: (0, 0, 1), 1: (1, 1, 31), 2: (0, 1, 3), 3: (0, 1, 7), 4: (0, 1, 11), 5: (1, 0, 16), 6: (1, 1, 5)}
PROTECT_INDEX = {0: 0, 1: 1, 2: 65535, 3: 65536, 4: 2 ** 31 - 1, 6: 2 ** 31, 7: 2 ** 31 - 2, 8: 12345678}


def test_protect_against_the_model(host):
    n = 12
    rng = np.random.default_rng(11)
    X, Y = sessions(n)
    X.bound[9] = 0
    keys = M.random_keys(rng, range(n), no_tx=(5,))
    h, model = pair(host, rng, n, PROTECT_SHAPES)
    ses = HostSes(host, X, keys, tx_state=PROTECT_INDEX)
    tx_state = {s: PROTECT_INDEX.get(s, 0) for s in range(n)}
    streams = list(range(n))
    for call in range(3):
        # the first call's cap cuts the last listed packet: its trailer's end is one byte beyond
        need = M.model_build_trailer(__import__("copy").deepcopy(model), X, Y, streams, NOW + call, 2 ** 40, 14)[3]["bytes_needed"]
        cap = need - 1 if call == 0 else need
        dg, wire, cnt, c = both_build(h, model, X, Y, streams, NOW + call, cap, 14, room=need)
        if call == 0:
            assert sorted(int(d[1]) for d in dg[:7]) == [20, 48, 52, 56, 56, 68, 96] and dg[11][1] == 0 and dg[9][1] == 0
        dg_all = np.full((n + 2, 2), FILL32, np.int32)
        dg_all[:n] = dg
        want = M.model_protect(keys, tx_state, n, streams, False, dg, wire)
        r, got = ses.protect(streams, cnt, dg_all, wire)
        assert r == 0 and got == want["count"], (got, want["count"])
        assert np.array_equal(dg_all[:n], want["dgrams"]) and (dg_all[n:] == FILL32).all() and np.array_equal(wire, want["wire"])
        tx_state = want["tx_state"]
        assert ses.index() == ([tx_state[s] for s in range(n)], [-1] * n)
        if call == 0:
            assert got == dict(count_dict([0] * 8), ok=8, skipped=2, no_key=1, exhausted=1)
            assert tx_state[4] == 2 ** 31 and tx_state[6] == 2 ** 31 and dg_all[6].tolist() == [0, 0] and dg_all[5].tolist() == [0, 0]
            for s in (0, 1, 2, 3, 4):                                  # the word behind the packet: E and the index the stream stood at
                off, ln = (int(v) for v in dg_all[s])
                assert int.from_bytes(wire[off + ln - 14:off + ln - 10].tobytes(), "big") == 0x80000000 | PROTECT_INDEX[s]
        if call == 1:
            assert got["exhausted"] == 2 and got["ok"] == 8            # stream 4 has used its last index, stream 11 is no longer cut
    # a refused list: ok = -1, nothing touched
    before = ses.snapshot()
    dgr, wr, cntr, _ = both_build(h, model, X, Y, [3, 2], NOW, 2 ** 40, 14)
    dg_all, wire = np.array([[0, 48], [48, 48]], np.int32), aligned_bytes(208)
    wire[:] = rng.integers(0, 256, 208, dtype=np.uint8)
    keep = wire.copy()
    r, got = ses.protect([3, 2], cntr, dg_all, wire)
    assert r == 0 and got == dict(count_dict([0] * 8), ok=-1) and np.array_equal(wire, keep) and dg_all.tolist() == [[0, 48], [48, 48]] and ses.snapshot() == before
    # malformed: a length that is no multiple of 4 or below 8, a range whose trailer reaches past wire_bytes, a stream outside the session
    ok_cnt = np.zeros(8, np.int32)
    for dgs, st, wb in (([[0, 50]], [1], 200), ([[0, 4]], [1], 200), ([[100, 88]], [1], 201), ([[-4, 48]], [1], 200), ([[0, 48]], [n], 200)):
        dg_all = np.array(dgs, np.int32)
        r, got = ses.protect(st, ok_cnt, dg_all, wire, wire_bytes=wb)
        assert r == 0 and got == dict(count_dict([0] * 8), malformed=1) and dg_all.tolist() == [[0, 0]] and np.array_equal(wire, keep) and ses.snapshot() == before
    dg_all = np.array([[100, 88]], np.int32)
    assert ses.protect([1], ok_cnt, dg_all, wire, wire_bytes=202)[1]["ok"] == 1 and dg_all.tolist() == [[100, 102]]
    # the argument rules
    dg_all = np.array([[0, 48]], np.int32)
    for kw in (dict(trailer=13), dict(rtcp_streams=n + 1), dict(wire_bytes=-1)):
        assert ses.protect([1], ok_cnt, dg_all, wire, **kw)[0] == -1
    assert ses.protect(list(range(n)) + [0], ok_cnt, np.zeros((n + 1, 2), np.int32), wire)[0] == -1
    assert ses.protect([1], ok_cnt, dg_all, wire[1:])[0] == -1 and ses.protect([1], ok_cnt[1:], dg_all, wire)[0] == -1
    h.close()
    ses.close()


def test_protect_without_any_key(host):
    X, _ = sessions(4)
    ses = HostSes(host, X)
    wire, dg = aligned_bytes(64), np.array([[0, 20]], np.int32)
    assert ses.protect([2], np.zeros(8, np.int32), dg, wire)[1] == dict(count_dict([0] * 8), no_key=1) and dg.tolist() == [[0, 0]] and (wire == FILL8).all()
    assert ses.unprotect(np.array([[0, 40]], np.int32), wire)[1]["unknown_ssrc"] == 1 and ses.index() == ([0] * 4, [-1] * 4)
    ses.close()


# ---- unprotect ---------------------------------------------------------------------------------------------------------------------------------
def receiving_session(n, hostile):
    """the peers' session, with the four streams behind `hostile` bound one SSRC bit away from it"""
    _, Y = sessions(n)
    for k, x in enumerate(M.twin_ssrcs(Y.ssrc[hostile])):
        Y.ssrc[hostile + 1 + k] = x
    return Y


def receive_case(rng, n=12, hostile=2):
    Y = receiving_session(n, hostile)
    Y.bound[10] = 0
    keys = M.random_keys(rng, range(n), no_rx=(8,))
    rx_state = {s: -1 for s in range(n)}
    rx_state.update({hostile: 1000, 7: 2 ** 31 - 2, 9: 65535})
    items = M.hostile_set(R, rng, Y, keys, rx_state, hostile, 1001)
    for s, index in ((0, 0), (1, 2 ** 31 - 1), (7, 2 ** 31 - 1), (9, 65536), (11, 5)):
        items.append(("stream_%d" % s, M.protect_packet(M.session_keys(keys[s]["rx"]), R.write_rr(Y.ssrc[s]) + R.write_sdes(Y.ssrc[s], b"s%d" % s), index), "ok"))
    items.append(("no_key", M.protect_packet(M.session_keys(bytes(30)), R.write_rr(Y.ssrc[8]), 3), "no_key"))
    items.append(("unbound", M.protect_packet(M.session_keys(keys[10]["rx"]), R.write_rr(Y.ssrc[10]), 3), "unknown_ssrc"))
    items.append(("record_at_the_end", M.protect_packet(M.session_keys(keys[7]["rx"]), R.write_rr(Y.ssrc[7]), 2 ** 31 - 2), "replayed"))
    order = rng.permutation(len(items))
    return Y, keys, rx_state, [items[i] for i in order]


@pytest.mark.parametrize("align", [0, 1, 2, 3])
def test_unprotect_against_the_model(host, align):
    rng = np.random.default_rng(21)
    Y, keys, rx_state, items = receive_case(rng)
    names = [k[0] for k in items]
    assert {"flip_byte_4", "flip_byte_7", "len_21", "len_22", "copy_a", "copy_b", "e0", "flip_e", "flip_index", "equal_to_record", "below_record", "large"} <= set(names)
    dg, wire = M.lay_out(rng, [k[1] for k in items], align=[align])
    assert all(int(o) % 4 == align for o in dg[:, 0])
    dg = np.concatenate([dg, np.array([[wire.size - 10, 40], [-4, 30], [wire.size, 22]], np.int32)])
    want = M.model_unprotect(Y, keys, rx_state, dg, wire)
    assert want["verdicts"][:len(items)] == [k[2] for k in items], [(k[0], k[2], v) for k, v in zip(items, want["verdicts"]) if k[2] != v]
    assert all(want["verdicts"][names.index("flip_byte_%d" % b)] == "auth_failed" for b in range(8)) and want["verdicts"][-3:] == ["malformed"] * 3
    ses = HostSes(host, Y, keys, rx_state=rx_state)
    w = wire.copy()
    out, cnt = ses.unprotect(dg, w)
    assert cnt == want["count"], (cnt, want["count"])
    assert np.array_equal(out, want["dgrams"]) and np.array_equal(w, want["wire"])
    for (off, ln), v in zip(dg.tolist()[:len(items)], want["verdicts"]):                      # a rejected datagram keeps every byte
        assert v == "ok" or np.array_equal(w[off:off + ln], wire[off:off + ln])
    assert ses.index()[1] == [want["rx_state"][s] for s in range(Y.n)]
    # every accepted datagram parses as the compound packet that went in
    for (name, d, v), (off, ln) in zip(items, out.tolist()):
        if v == "ok" and not name.startswith("odd") and name != "bare_rr":
            assert R.read_compound(w[off:off + ln].tobytes())[0] == "accepted", name
    # the same call again: what was accepted is now replayed, every byte kept
    w2 = w.copy()
    out2, cnt2 = ses.unprotect(dg, w2)
    again = M.model_unprotect(Y, keys, want["rx_state"], dg, w)
    assert cnt2 == again["count"] and cnt2["ok"] == 0 and cnt2["replayed"] >= want["count"]["ok"] and np.array_equal(w2, w) and not out2.any()
    ses.close()


def test_batch_and_sequential_receivers(host):
    """equal whenever a stream's datagrams stand in increasing index order in the call -- so whenever a call holds at most one datagram per
    stream --; the batch result is the same under any permutation of the call"""
    rng = np.random.default_rng(31)
    n = 9
    _, Y = sessions(n)
    keys = M.random_keys(rng, range(n))
    rx_state = {s: int(rng.integers(-1, 50)) for s in range(n)}
    ses = HostSes(host, Y, keys, rx_state=rx_state)
    state = dict(rx_state)
    for call in range(6):
        per_stream = call < 3                                         # one datagram per stream, then several in increasing order
        packets = []
        for s in range(n):
            base = state[s] + int(rng.integers(-3, 4))
            for index in sorted({max(0, base + int(rng.integers(0, 6))) for _ in range(1 if per_stream else 3)}):
                packets.append((s, M.protect_packet(M.session_keys(keys[s]["rx"]), R.write_rr(Y.ssrc[s]) + R.write_sdes(Y.ssrc[s], b"x" * (1 + s)), index)))
        slot = rng.random(len(packets))                               # any interleaving of the streams ...
        if not per_stream:                                            # ... that keeps each stream's datagrams in increasing index order
            for s in range(n):
                mine = [i for i, q in enumerate(packets) if q[0] == s]
                slot[mine] = np.sort(slot[mine])
        order = np.argsort(slot)
        dg, wire = M.lay_out(rng, [packets[i][1] for i in order])
        batch, seq = M.model_unprotect(Y, keys, state, dg, wire), M.sequential_unprotect(Y, keys, state, dg, wire)
        assert batch["verdicts"] == seq["verdicts"] and batch["rx_state"] == seq["rx_state"] and np.array_equal(batch["wire"], seq["wire"])
        assert 0 < batch["count"]["replayed"] and 0 < batch["count"]["ok"]
        # a permutation of the call: the same verdict for every datagram, the same records
        perm = rng.permutation(len(order))
        other = M.model_unprotect(Y, keys, state, dg[perm], wire)
        assert [other["verdicts"][k] for k in np.argsort(perm)] == batch["verdicts"] and other["rx_state"] == batch["rx_state"]
        w = wire.copy()
        out, cnt = ses.unprotect(dg[perm], w)
        assert cnt == other["count"] and np.array_equal(out, other["dgrams"]) and np.array_equal(w, other["wire"])
        state = batch["rx_state"]
        assert ses.index()[1] == [state[s] for s in range(n)]
    # where they differ: a newer datagram in front of an older one of the same stream -- the batch takes both, and says so in the header
    s, k = 0, M.session_keys(keys[0]["rx"])
    two = [M.protect_packet(k, R.write_rr(Y.ssrc[s]), state[s] + 2), M.protect_packet(k, R.write_rr(Y.ssrc[s]), state[s] + 1)]
    dg, wire = M.lay_out(rng, two)
    assert M.model_unprotect(Y, keys, state, dg, wire)["verdicts"] == ["ok", "ok"] and M.sequential_unprotect(Y, keys, state, dg, wire)["verdicts"] == ["ok", "replayed"]
    assert ses.unprotect(dg, wire.copy())[1]["ok"] == 2 and ses.index([0])[1] == [state[0] + 2]
    ses.close()


# ---- the loop ----------------------------------------------------------------------------------------------------------------------------------
def test_secured_loop_equals_the_loop_in_the_clear(host):
    """build, protect, unprotect, parse gives the feedback and the state of build, parse"""
    n = 30
    rng = np.random.default_rng(41)
    X, Y = sessions(n)
    keys = M.random_keys(rng, range(n))
    A, mA = pair(host, rng, n)
    B, mB = pair(host, np.random.default_rng(42), n)
    A2, B2 = HostRtcp(host, n), HostRtcp(host, n)
    A2.set_words(A.words())
    B2.set_words(B.words())
    tx, rx = HostSes(host, X, keys), HostSes(host, X, M.loop_keys(keys))
    streams = list(range(0, n, 2)) + [n - 1]
    for tick in range(3):
        now = NOW + (tick << 32)
        dg, wire, cnt, c = both_build(A, mA, X, Y, streams, now, 2 ** 40, 14)
        A2.trailer = 0
        _, dgp, wirep, _, cp = A2.build(X, Y, streams, now, 2 ** 40)
        assert cp["built"] == c["built"] and c["bytes"] > cp["bytes"]
        r, pc = tx.protect(streams, cnt, dg, wire)
        assert r == 0 and pc["ok"] == len(streams)
        for (off, ln), (po, pl) in zip(dg.tolist(), dgp.tolist()):    # no cleartext body byte survives
            assert ln == pl + 14 and np.array_equal(wire[off:off + 8], wirep[po:po + 8])
            assert pl <= 8 or not np.array_equal(wire[off + 8:off + pl], wirep[po + 8:po + pl])
        moved = rng.integers(0, 256, wire.size + 3, dtype=np.uint8)    # the receiver's buffer: another alignment
        moved[3:] = wire
        dgr = dg + np.array([3, 0], np.int32)
        out, uc = rx.unprotect(dgr, moved)
        assert uc["ok"] == len(streams)
        fb, c1 = B.parse(X, Y, out, moved, now + 5)
        fb2, c2 = B2.parse(X, Y, dgp, wirep, now + 5)
        assert c1 == c2 and np.array_equal(fb, fb2) and np.array_equal(B.words(), B2.words()) and np.array_equal(A.words(), A2.words())
        assert tx.index(streams)[0] == [tick + 1] * len(streams) and rx.index(streams)[1] == [tick] * len(streams)
    for o in (A, B, A2, B2, tx, rx):
        o.close()


# ---- the control plane -------------------------------------------------------------------------------------------------------------------------
def test_control_plane(host):
    n = 6
    X, _ = sessions(n)
    rng = np.random.default_rng(51)
    key = [rng.integers(0, 256, 30, dtype=np.uint8).tobytes() for _ in range(4)]
    ses = HostSes(host, X)
    assert ses.snapshot() == b"" and ses.index() == ([0] * n, [-1] * n)            # nothing is allocated before the first key
    assert ses.set_keys([1, 3], tx=key[:2], rx=key[2:], tx_index=[7, 2 ** 31], rx_index=[-1, 2 ** 31 - 1]) == 0
    assert len(ses.snapshot()) == 532 * n + 2 * n
    assert ses.index() == ([0, 7, 0, 2 ** 31, 0, 0], [-1, -1, -1, 2 ** 31 - 1, -1, -1])
    before = ses.snapshot()
    for kw in (dict(streams=[], tx=[]), dict(streams=[n], tx=key[:1]), dict(streams=[-1], tx=key[:1]), dict(streams=[1, 1], tx=key[:2]), dict(streams=[1]),
               dict(streams=[1], tx=key[:1], tx_index=[2 ** 31 + 1]), dict(streams=[1], rx=key[:1], rx_index=[-2]), dict(streams=[1], rx=key[:1], rx_index=[2 ** 31]),
               dict(streams=[1], tx=key[:1], rx_index=[2 ** 31])):
        assert ses.set_keys(**kw) == -1 and ses.snapshot() == before, kw
    for bad in ([], [n], [0, 0]):
        assert ses.clear_keys(bad) == -1 and ses.unbind(bad) == -1 and ses.snapshot() == before
    # a NULL direction keeps what it had: key, index and mirror
    w1 = host.emu_srtcp_key_words(ses.h, 1)
    assert ses.set_keys([1], rx=key[3:4], rx_index=[40]) == 0
    after = ses.snapshot()
    assert ses.index([1]) == ([7], [40]) and after[:256] == before[:256] and after[512:768] == before[512:768] and after[768:1024] != before[768:1024]
    assert host.emu_srtcp_key_words(ses.h, 1) == w1 and after[532 * n:] == before[532 * n:]
    assert ses.set_keys([1], tx=key[3:4]) == 0 and ses.index([1]) == ([0], [40])      # a tx key sets the send index: NULL = 0
    # clear_keys and unbind wipe keys, indices and mirror
    assert ses.clear_keys([1]) == 0 and host.emu_srtcp_key_words(ses.h, 1) == 0 and ses.index([1]) == ([0], [-1])
    assert host.emu_srtcp_key_words(ses.h, 3) > 100
    assert ses.unbind([3]) == 0 and host.emu_srtcp_key_words(ses.h, 3) == 0 and ses.index([3]) == ([0], [-1])
    fresh = np.zeros(532 * n + 2 * n, np.uint8)
    fresh[512 * n:528 * n].view(np.int64)[0::2] = -1
    assert ses.snapshot() == fresh.tobytes()
    assert [host.emu_srtcp_trailer_ok(t) for t in (-1, 0, 14, 16, 17)] == [-1, 0, 0, 0, -1]
    ses.close()


# ---- ABI, binding --------------------------------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_listed_and_bound(host):
    import solo_amd
    hdr = T.header_text()
    lib = T.built_library()
    bound = solo_amd.load_library()
    for name, n_args in SRTCP_SYMBOLS.items():
        assert name in solo_amd.ABI_SYMBOLS and (name + "(") in hdr.replace(" (", "("), name
        assert hasattr(lib, name), name
        assert len(getattr(bound, name).argtypes) == n_args and getattr(bound, name).restype is C.c_int32, name
    assert bound.solo_srtcp_protect.argtypes[7] is C.c_int64 and bound.solo_srtcp_unprotect.argtypes[4] is C.c_int64
    assert "#define SOLO_SRTCP_TRAILER_BYTES 14" in hdr and solo_amd.SRTCP_TRAILER_BYTES == 14 == M.TRAILER
    assert C.sizeof(solo_amd.solo_srtcp_count_t) == 32 == host.emu_srtcp_sizes(0) and "solo_srtcp_count_t;" in hdr
    assert [f for f, _ in solo_amd.solo_srtcp_count_t._fields_] == list(M.VERDICTS)
    assert re.search(r"int32_t ok, skipped, malformed, unknown_ssrc, no_key, auth_failed, replayed, exhausted; \} solo_srtcp_count_t;", hdr)
    assert [host.emu_srtcp_sizes(k) for k in range(1, 6)] == [256, 16, 4, 14, 532]
    for m in ("set_rtcp_keys", "clear_rtcp_keys", "rtcp_index", "protect_rtcp", "unprotect_rtcp", "srtcp_count"):
        assert callable(getattr(solo_amd.Rtp, m)), m
    assert callable(solo_amd.Rtcp.set_trailer)
    src = open(os.path.join(T.ROOT, "solo_amd", "csrc", "solo_srtcp.h")).read()
    assert "typedef solo_srtcp_count_t SxSrtcpCount;" in src and "static_assert(sizeof(SxSrtcpCount) == 32" in src
    srtp = open(os.path.join(T.ROOT, "solo_amd", "csrc", "solo_srtp.h")).read()
    assert "sizeof(SxSrtpKey) == 256" in srtp and "struct SxSrtpKey" not in src                  # the key record is SRTP's, as it is
    for name in ("sx_aes_cm_block", "sx_srtp_cipher", "sx_srtp_mac", "sx_srtp_tag_byte"):        # used, not copied
        assert len(re.findall(r"SX_HD \w+ %s\(" % name, srtp)) == 1 and not re.search(r"SX_HD \w+ %s\(" % name, src), name


def test_capture_claims_name_a_test():
    """the header's SRTCP block calls the two device calls capturable and names the tests of tests/test_gpu_srtcp.py that capture them"""
    import test_gpu_srtcp as GPU
    text = open(os.path.join(T.ROOT, "include", "solo_mi355x.h")).read()
    m = re.search(r"/\* SRTCP \(RFC 3711 section 3\.4\).*?\*/", text, flags=re.S)
    assert m and m.group(0).count("capturable") == 2 and "solo_rtcp_set_trailer" in m.group(0) and "STRICTLY NEWER" in m.group(0)
    tests = {x.name for x in ast.parse(open(GPU.__file__).read()).body if isinstance(x, ast.FunctionDef) and x.name.startswith("test_")}
    assert set(GPU.CAPTURED) == {"solo_srtcp_protect", "solo_srtcp_unprotect"} and set(GPU.CAPTURED.values()) <= tests
    for name in GPU.CAPTURED.values():
        assert "tests/test_gpu_srtcp.py: %s" % name in m.group(0), name
    # the blocks beside it keep their claims, and no longer list SRTCP as not built
    srtp = re.search(r"/\* SRTP at both ends.*?\*/", text, flags=re.S).group(0)
    rtcp = re.search(r"/\* RTCP \(RFC 3550 section 6\.4\).*?\*/", text, flags=re.S).group(0)
    assert srtp.count("capturable") == 3 and rtcp.count("capturable") == 4
    assert "SRTCP" not in srtp.split("Not built")[1] and "SRTCP" not in rtcp.split("Not built")[1]
    assert "on the host until" not in open(os.path.join(T.ROOT, "INTEGRATION.md")).read()


def test_binding_checks():
    import solo_amd
    torch = pytest.importorskip("torch")
    o = object.__new__(solo_amd.Rtp)
    o.n_rows = o.n_streams = 8
    o.packet_samples, o.level_id, o.trailer = 640, 0, 0
    o.torch, o.lib, o.h, o.device = torch, T.NoLib(), None, torch.device("cpu")
    o._stream = lambda: None
    c = object.__new__(solo_amd.Rtcp)
    c.n_rows = c.n_streams = 8
    c.trailer, c.torch, c.lib, c.h, c.device = 14, torch, T.NoLib(), 1, torch.device("cpu")
    c._stream = lambda: None
    for bad in (-1, 17, "x"):
        with pytest.raises(ValueError):
            c.set_trailer(bad)
    k = bytes(30)
    for kw in (dict(streams=[0, 0], tx=[k, k]), dict(streams=[8], tx=[k]), dict(streams=[0], tx=[k[:29]]), dict(streams=[0]), dict(streams=[0, 1], rx=[k]),
               dict(streams=[0], tx=[k], tx_index=2 ** 31 + 1), dict(streams=[0], tx=[k], tx_index=-1), dict(streams=[0], rx=[k], rx_index=-2),
               dict(streams=[0], rx=[k], rx_index=2 ** 31), dict(streams=[0], rx=[k], rx_index=[1, 2]), dict(streams=[0], rx=[k], rx_index="x")):
        with pytest.raises(ValueError):
            o.set_rtcp_keys(**kw)
    for lst in ([], [8], [0, 0]):
        with pytest.raises(ValueError):
            o.clear_rtcp_keys(lst)
        with pytest.raises(ValueError):
            o.rtcp_index(lst)
    D = T.FakeDev
    I32, U8 = torch.int32, torch.uint8
    good = dict(rtcp=c, streams=D((5,), I32), build_count=D((8,), I32), dgrams=D((5, 2), I32), wire=D((999,), U8))
    c13 = object.__new__(solo_amd.Rtcp)
    c13.n_rows = c13.n_streams = 8
    c13.trailer, c13.h = 13, 1
    c9 = object.__new__(solo_amd.Rtcp)
    c9.n_rows = c9.n_streams = 9
    c9.trailer, c9.h = 14, 1
    for over in (dict(rtcp=None), dict(rtcp=c13), dict(rtcp=c9), dict(streams=[0, 1, 2, 3, 4]), dict(streams=D((0,), I32), dgrams=D((0, 2), I32)),
                 dict(streams=D((9,), I32), dgrams=D((9, 2), I32)), dict(build_count=D((6,), I32)), dict(dgrams=D((4, 2), I32)), dict(dgrams=None),
                 dict(wire=D((999,), I32)), dict(wire=D((999,), U8, cuda=False)), dict(wire=D((999,), U8, contiguous=False))):
        with pytest.raises(ValueError):
            o.protect_rtcp(**dict(good, **over))
    good = dict(dgrams=D((10, 2), I32), wire=D((999,), U8), dgrams_out=D((10, 2), I32))
    for over in (dict(dgrams=D((10, 3), I32)), dict(wire=D((9, 9), U8)), dict(dgrams_out=D((9, 2), I32)), dict(dgrams_out=D((10, 2), I32, cuda=False)), dict(wire=None)):
        with pytest.raises(ValueError):
            o.unprotect_rtcp(**dict(good, **over))
    c.h = c13.h = c9.h = None


# ---- the built library's kernels ------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="no LLVM binutils on this box")
def test_srtcp_kernels_use_no_scratch():
    import solo_amd
    T.built_library()
    sys.path.insert(0, os.path.join(T.ROOT, "tools"))
    from kernel_resources import kernel_resources
    seen = kernel_resources(solo_amd.LIB_PATH)
    for frag in KERNELS:
        hits = [r for name, r in seen.items() if frag in name]
        assert len(hits) == 1, (frag, len(hits))
        assert hits[0]["scratch"] == 0, (frag, hits[0])


# ---- the same source as a stand-alone program under the sanitisers -----------------------------------------------------------------------------------
def test_stand_alone_build_under_the_sanitisers(tmp_path):
    """tests/srtcp_host.cpp with its own main, -fsanitize=address,undefined: the hostile family in through a file, in heap blocks of exactly
    their size, every output back through a file and against the model; any report of a sanitiser ends the program with a non-zero status"""
    exe = str(tmp_path / "srtcp_asan")
    flags = [f for f in FLAGS if f not in ("-shared", "-fPIC", "-O2")] + ["-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                                                         "-DSRTCP_MAIN"]
    cxx = os.environ.get("CXX", "g++")
    if os.path.basename(cxx).startswith("g++"):                       # the runtimes inside the program: nothing has to load ahead of it
        flags += ["-static-libasan", "-static-libubsan"]
    subprocess.check_call([cxx] + flags + [source("srtcp"), "-o", exe])
    for seed in (61, 62):
        rng = np.random.default_rng(seed)
        Y, keys, rx_state, items = receive_case(rng)
        for s in (8, 10):                                              # (the program keys and binds every stream)
            keys[s]["rx"] = keys[s]["rx"] or rng.integers(0, 256, 30, dtype=np.uint8).tobytes()
        Y.bound[10] = 1
        dg, wire = M.lay_out(rng, [k[1] for k in items], front=seed & 3, gap=0)
        wire = wire[:int(dg[-1].sum())]                               # the last datagram ends with the block
        dg = np.concatenate([dg, np.array([[wire.size - 10, 40], [-4, 30], [wire.size, 22]], np.int32)])
        want = M.model_unprotect(Y, keys, rx_state, dg, wire)
        assert want["count"]["ok"] > 10 and want["count"]["auth_failed"] > 10 and want["count"]["replayed"] >= 3 and want["count"]["malformed"] >= 5
        fin, fout = str(tmp_path / ("in%d.bin" % seed)), str(tmp_path / ("out%d.bin" % seed))
        with open(fin, "wb") as f:
            f.write(np.array([Y.n, dg.shape[0], wire.size, 0, 0, 0, 0, 0], np.int32).tobytes())
            f.write(np.array(Y.ssrc, np.uint32).tobytes())
            f.write(np.array([rx_state[s] for s in range(Y.n)], np.int64).tobytes())
            f.write(b"".join(keys[s]["rx"] for s in range(Y.n)))
            f.write(dg.tobytes())
            f.write(wire.tobytes())
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        raw = open(fout, "rb").read()
        n = dg.shape[0]
        out = np.frombuffer(raw[:8 * n], np.int32).reshape(n, 2)
        cnt = np.frombuffer(raw[8 * n:8 * n + 32], np.int32)
        index = np.frombuffer(raw[8 * n + 32:8 * n + 32 + 8 * Y.n], np.int64)
        w = np.frombuffer(raw[8 * n + 32 + 8 * Y.n:], np.uint8)
        assert count_dict(cnt) == want["count"] and np.array_equal(out, want["dgrams"]) and np.array_equal(w, want["wire"])
        assert index.tolist() == [want["rx_state"][s] for s in range(Y.n)]

"""RTCP (solo_rtcp_*, solo_amd/csrc/solo_rtcp.h) without a GPU: the passes are compiled for the host by this test (tests/rtcp_host.cpp,
through tests/host_build.py) and compared with the independent model of tests/rtcp_model.py, state word for state word, wire byte for
wire byte and count for count after every tick of the scenarios the GPU runs as well (tests/test_gpu_rtcp.py), with guard bytes behind
every output; then the wire format against byte literals, the model's own properties, the argument rules, the ABI and the binding."""
import ast
import ctypes as C
import os
import re

import numpy as np
import pytest

import rtcp_model as M
import solo_testlib as T
from host_build import host_lib

RTCP_SYMBOLS = ("solo_rtcp_create", "solo_rtcp_destroy", "solo_rtcp_reset", "solo_rtcp_reset_rows", "solo_rtcp_get_state", "solo_rtcp_set_state",
                "solo_rtcp_set_cname", "solo_rtcp_received", "solo_rtcp_sent", "solo_rtcp_build", "solo_rtcp_parse")
FILL8, FILL32 = 0xA5, -7
L = 640
VP, I, U64 = C.c_void_p, C.c_int, C.c_uint64


@pytest.fixture(scope="module")
def host():
    lib = host_lib("rtcp")
    lib.emu_rtcp_create.restype = VP
    lib.emu_rtcp_create.argtypes = [I]
    lib.emu_rtcp_destroy.argtypes = [VP]
    lib.emu_rtcp_reset_rows.argtypes = [VP, VP, I]
    lib.emu_rtcp_state.argtypes = [VP, VP, I]
    lib.emu_rtcp_set_cname.argtypes = [VP, VP, I, VP]
    lib.emu_rtcp_table.argtypes = [VP, I, VP]
    lib.emu_rtcp_received.argtypes = [VP, VP, I, I, VP, VP, I, VP, C.c_uint, VP]
    lib.emu_rtcp_sent.argtypes = [VP, I, VP, VP, I, VP, VP]
    lib.emu_rtcp_build.argtypes = [VP, VP, I, I, VP, I, VP, I, U64, VP, VP, VP, C.c_longlong, VP]
    lib.emu_rtcp_parse.argtypes = [VP, VP, I, VP, I, VP, I, VP, C.c_longlong, U64, VP, VP, VP]
    return lib


def p(x):
    return None if x is None else x.ctypes.data


def check(ok, msg):
    assert ok, msg


def count_of(fields, a):
    return dict(zip(fields, (int(v) for v in a)))


def build_count_of(a):
    return dict(built=int(a[0]), built_needed=int(a[1]), bytes=int(a[2:4].view(np.int64)[0]), bytes_needed=int(a[4:6].view(np.int64)[0]),
                refused=int(a[6]), with_sr=int(a[7]))


class HostRtcp:
    """the host form's object, with the interface the drivers of tests/rtcp_model.py call"""

    def __init__(self, lib, n):
        self.lib, self.n = lib, n
        self.h = lib.emu_rtcp_create(n)
        assert self.h

    def table(self, session):
        cfg, t = session.cfg(), np.zeros(4 + 2 * session.n, np.uint32)
        assert self.lib.emu_rtcp_table(p(cfg), session.n, p(t)) == 0
        return t

    def words(self):
        w = np.zeros((self.n, 40), np.uint32)
        self.lib.emu_rtcp_state(self.h, p(w), 0)
        return w

    def set_words(self, w):
        w = np.ascontiguousarray(w, np.uint32)
        assert w.shape == (self.n, 40)
        self.lib.emu_rtcp_state(self.h, p(w), 1)

    def set_cname(self, streams, names):
        idx = np.asarray(streams, np.int32)
        buf = np.frombuffer(b"".join(bytes(x).ljust(32, b"\0")[:32] for x in names), np.uint8).copy()
        return self.lib.emu_rtcp_set_cname(self.h, p(idx), len(idx), p(buf))

    def received(self, session, tick):
        arr, cfg = tick["arrivals"], session.cfg()
        cnt = np.full(8 + 4, FILL32, np.int32)
        r = self.lib.emu_rtcp_received(self.h, p(cfg), session.n, session.L, p(arr), p(tick["rtp_seq"]), arr.shape[0], p(tick["arrival_time"]), tick["now_rtp"],
                                       p(cnt))
        assert r == 0 and (cnt[8:] == FILL32).all() and cnt[7] == 0
        return count_of(M.RECEIVED_COUNT, cnt)

    def sent(self, session, rec, n_rec, dg):
        sc, cnt = np.array([n_rec, n_rec, 0, 0, 0, 0, 0, 0], np.int32), np.full(8 + 4, FILL32, np.int32)
        assert self.lib.emu_rtcp_sent(self.h, session.n, p(rec), p(sc), rec.shape[0], p(dg), p(cnt)) == 0
        assert (cnt[8:] == FILL32).all() and (cnt[2:8] == 0).all()
        return count_of(M.SENT_COUNT, cnt)

    def build(self, tx, rx, streams, now, cap, guard=64):
        idx = np.asarray(streams, np.int32)
        room = int(min(cap, 96 * len(idx)))
        dg, wire, cnt = np.full((len(idx) + 2, 2), FILL32, np.int32), np.full(room + guard, FILL8, np.uint8), np.full(8 + 4, FILL32, np.int32)
        ctx, crx = tx.cfg(), None if rx is None else rx.cfg()
        r = self.lib.emu_rtcp_build(self.h, p(ctx), tx.n, tx.L, p(crx), 0 if rx is None else rx.n, p(idx), len(idx), now, None, p(dg), p(wire), cap, p(cnt))
        assert (cnt[8:] == FILL32).all() and (dg[len(idx):] == FILL32).all() and (wire[room:] == FILL8).all()
        if r == 1:
            assert (dg == FILL32).all() and (wire == FILL8).all() and (cnt[1:] == FILL32).all()
            return r, dg[:len(idx)], wire, dict(built=int(cnt[0]))
        c = build_count_of(cnt)
        assert (wire[c["bytes"]:] == FILL8).all()           # nothing at or beyond what was written, the cap included
        return r, dg[:len(idx)], wire, c

    def parse(self, rx, tx, dgrams, wire, now):
        fb, cnt = np.full((self.n + 1, 8), 0xA5A5A5A5, np.uint32), np.full(16 + 4, FILL32, np.int32)
        trx, ttx = self.table(rx), None if tx is None else self.table(tx)
        wire = np.ascontiguousarray(wire)
        r = self.lib.emu_rtcp_parse(self.h, p(trx), rx.n, p(ttx), 0 if tx is None else tx.n, p(dgrams), dgrams.shape[0], p(wire), wire.shape[0], now, None,
                                    p(fb), p(cnt))
        assert r == 0 and (cnt[16:] == FILL32).all() and (cnt[10:16] == 0).all() and (fb[self.n] == 0xA5A5A5A5).all()
        return fb[:self.n].copy(), count_of(M.PARSE_COUNT, cnt)

    def close(self):
        self.lib.emu_rtcp_destroy(self.h)


def sessions(n, seq_offset=None):
    """X (side A's own streams) and Y (side B's): SSRCs in no order, timestamp offsets near the wrap"""
    X = M.Session([0x10000000 + (s * 2654435761) % 0xFFFFF for s in range(n)], [(0xFFFFF000 + 977 * s) & M.M32 for s in range(n)], packet_samples=L)
    Y = M.Session([0xE0000000 - 31 * s * s - s for s in range(n)], [12345 * s for s in range(n)], packet_samples=L)
    return X, Y


# ---- structure sizes, ABI, binding -------------------------------------------------------------------------------------------------------
def test_structure_sizes(host):
    import solo_amd
    want = (128, 32, 32, 32, 64, 32, 128, 32, 128)
    assert tuple(host.emu_rtcp_sizes(k) for k in range(9)) == want
    for name, size in (("received_count", 32), ("sent_count", 32), ("build_count", 32), ("parse_count", 64), ("feedback", 32)):
        assert C.sizeof(getattr(solo_amd, "solo_rtcp_%s_t" % name)) == size
    assert [f for f, _ in solo_amd.solo_rtcp_received_count_t._fields_][:7] == list(M.RECEIVED_COUNT)
    assert [f for f, _ in solo_amd.solo_rtcp_build_count_t._fields_] == list(M.BUILD_COUNT)
    assert [f for f, _ in solo_amd.solo_rtcp_parse_count_t._fields_][:10] == list(M.PARSE_COUNT)
    assert [f for f, _ in solo_amd.solo_rtcp_feedback_t._fields_] == list(M.FEEDBACK)
    assert solo_amd.solo_rtcp_build_count_t.bytes_needed.offset == 16 and solo_amd.solo_rtcp_feedback_t.rtt.offset == 28
    assert solo_amd.RTCP_STATE_BYTES == 128 and solo_amd.RTCP_CNAME_BYTES == 32 and solo_amd.Rtcp.state_bytes == 160
    assert solo_amd.RTCP_WALK_MAX == host.emu_rtcp_sizes(8) and solo_amd.RTCP_BYE == M.BYE_BIT
    hdr = T.header_text()
    assert "#define SOLO_RTCP_STATE_BYTES 128" in hdr and "#define SOLO_RTCP_CNAME_BYTES 32" in hdr and "#define SOLO_RTCP_WALK_MAX 128" in hdr
    src = open(os.path.join(T.ROOT, "solo_amd", "csrc", "solo_rtcp.h")).read()
    for rec in ("received_count", "sent_count", "build_count", "parse_count", "feedback"):
        assert "typedef solo_rtcp_%s_t SxRtcp" % rec in src                                     # each ABI record defined once


def test_symbols_declared_exported_and_bound():
    import solo_amd
    hdr = T.header_text()
    lib = T.built_library()
    for name in RTCP_SYMBOLS:
        assert name in solo_amd.ABI_SYMBOLS and (name + "(") in hdr.replace(" (", "("), name
        assert hasattr(lib, name), name
    bound = solo_amd.load_library()
    assert bound.solo_rtcp_create.restype is C.c_void_p and len(bound.solo_rtcp_create.argtypes) == 1
    assert [len(getattr(bound, "solo_rtcp_" + f).argtypes) for f in ("set_cname", "received", "sent", "build", "parse")] == [5, 9, 8, 12, 12]
    assert issubclass(solo_amd.Rtcp, solo_amd._RowStateObject)
    for m in ("set_cname", "received", "sent", "build", "parse", "count", "reset", "get_state", "set_state", "close"):
        assert callable(getattr(solo_amd.Rtcp, m)), m


def test_capture_claims_name_a_test():
    """the header calls the four device calls capturable: tests/test_gpu_rtcp.py names the test that captures each (its module loads
    without a GPU), and the header names that test"""
    import test_gpu_rtcp as GPU
    m = re.search(r"/\* RTCP \(RFC 3550 section 6\.4\).*?\*/", open(os.path.join(T.ROOT, "include", "solo_mi355x.h")).read(), flags=re.S)
    assert m and m.group(0).count("capturable") == 4
    tests = {n.name for n in ast.parse(open(GPU.__file__).read()).body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}
    assert set(GPU.CAPTURED) == {"solo_rtcp_received", "solo_rtcp_sent", "solo_rtcp_build", "solo_rtcp_parse"} and set(GPU.CAPTURED.values()) <= tests
    for name in GPU.CAPTURED.values():
        assert name in m.group(0), name


def test_binding_checks_arguments_before_the_library():
    """the argument checks go through the one checker of the binding: a bad argument is a ValueError, with no library and no GPU"""
    import solo_amd
    with pytest.raises(ValueError):
        solo_amd.Rtcp(0)
    o = object.__new__(solo_amd.Rtcp)
    o.n_rows = o.n_streams = 4
    o.h = None

    class FakeTorch:
        int32, int16, uint8, int64 = "i32", "i16", "u8", "i64"
    o.torch = FakeTorch
    for call in (lambda: o.received(None, np.zeros((3, 5)), None), lambda: o.sent(None, None, None, None), lambda: o.parse(None, None, None, None, 0),
                 lambda: o.set_cname([0, 0], b"a"), lambda: o.set_cname([0], b""), lambda: o.set_cname([0], b"x" * 32), lambda: o.set_cname([4], b"a"),
                 lambda: o.set_cname([0, 1], [b"a"]), lambda: o.count("other", None), lambda: o._now(-1), lambda: o._now(1 << 64),
                 lambda: o._session("rtp", object()), lambda: o.build(None, None, None, 0)):
        with pytest.raises(ValueError):
            call()


# ---- the wire format against byte literals ------------------------------------------------------------------------------------------------
SR_SDES = bytes.fromhex(
    "81c8000c" "11223344" "83aa7e80" "12345678" "0001f400" "00000007" "00000460"        # SR, RC 1, 12 words behind the first
    "aabbccdd" "40000003" "0001000a" "00000005" "7e801234" "00020000"                   # fraction 64, lost 3, cycle 1 seq 10, jitter 5, lsr, dlsr
    "81ca0003" "11223344" "01056140" "622e6300")                                        # SDES: CNAME "a@b.c", a zero, no pad
RR_SDES = bytes.fromhex("80c90001" "11223344" "81ca0004" "11223344" "01097573" "65724068" "6f737400")   # RR, RC 0; CNAME "user@host": nine bytes and the zero end a word


def literal_case(impl, model):
    """stream 0 in the state that SR_SDES describes: expected 65544, 3 lost; in the interval 4 expected, 1 lost; -> sessions"""
    tx = M.Session([0x11223344, 0x55], [0x1F400 - 3 * L, 0], packet_samples=L)
    rx = M.Session([0xAABBCCDD, 0x66], [0, 0], packet_samples=L)
    w = model.words()
    row = dict(base_seq=3, max_seq=10, cycles=65536, received=65541, expected_prior=65540, received_prior=65538, jitter=5 * 16 + 9, seen=7,
               lsr=0x7E801234, lsr_arrival=0x7E801234 - 0x20000, tx_packets=7, tx_octets=0x460, tx_next=3, tx_since=2, transit=99, bad_seq=65537)
    for k, f in enumerate(M.FIELDS):
        w[0, k] = row[f]
    model.set_words(w)
    impl.set_words(w)
    return tx, rx


def test_wire_format_against_literals(host):
    assert M.write_sr(0x11223344, 0x83AA7E8012345678, 0x1F400, 7, 0x460, [M.write_block(0xAABBCCDD, 64, 3, 0x1000A, 5, 0x7E801234, 0x20000)]) + \
        M.write_sdes(0x11223344, b"a@b.c") == SR_SDES
    assert M.write_rr(0x11223344) + M.write_sdes(0x11223344, b"user@host") == RR_SDES
    impl, model = HostRtcp(host, 2), M.Model(2)
    tx, rx = literal_case(impl, model)
    assert impl.set_cname([0], [b"a@b.c"]) == 0
    model.set_cname([0], [b"a@b.c"])
    r, dg, wire, c = impl.build(tx, rx, [0], 0x83AA7E8012345678, 1 << 20)
    assert r == 0 and dg.tolist() == [[0, len(SR_SDES)]] and bytes(wire[:len(SR_SDES)]) == SR_SDES, bytes(wire[:len(SR_SDES)]).hex()
    assert c == dict(built=1, built_needed=1, bytes=len(SR_SDES), bytes_needed=len(SR_SDES), refused=0, with_sr=1)
    assert model.build(tx, rx, [0], 0x83AA7E8012345678, 1 << 20)[2] == SR_SDES
    assert np.array_equal(impl.words(), model.words()) and model.rows[0]["expected_prior"] == 65544 and model.rows[0]["tx_since"] == 0
    # ... and read back by the peer: the literal's sender is known to it, its block is about the peer's own stream 0
    now = 0x83AA7E8412345678
    fb, c = impl.parse(tx, rx, np.array([[0, len(SR_SDES)]], np.int32), np.frombuffer(SR_SDES, np.uint8), now)
    assert c == M.Model(2).parse(tx, rx, [(0, len(SR_SDES))], SR_SDES, now)[1] and (c["accepted"], c["sr"], c["blocks"], c["skipped"]) == (1, 1, 1, 1)
    assert fb[0].tolist() == [1, 64, 3, 0x1000A, 5, 0x7E801234, 0x20000, 0x20000]
    assert fb[1].tolist() == [0, 0, 0, 0, 0, 0, 0, 0xFFFFFFFF]
    assert impl.words()[0, 10:12].tolist() == [0x7E801234, 0x7E841234]
    # an RR without a block
    impl2 = HostRtcp(host, 2)
    assert impl2.set_cname([0], [b"user@host"]) == 0
    r, dg, wire, c = impl2.build(tx, None, [0], 5, 1 << 20)
    assert r == 0 and bytes(wire[:c["bytes"]]) == RR_SDES and c["with_sr"] == 0
    fb, c = impl2.parse(tx, rx, np.array([[0, len(RR_SDES)]], np.int32), np.frombuffer(RR_SDES, np.uint8), now)
    assert (c["accepted"], c["sr"], c["blocks"], c["skipped"]) == (1, 0, 0, 1)
    impl.close()
    impl2.close()


# ---- the scenarios, every tick against the model ------------------------------------------------------------------------------------------
def fresh(host, n, names=True):
    impl, model = HostRtcp(host, n), M.Model(n)
    if names:
        cn = [b"s%d@example.net" % s for s in range(n)]
        assert impl.set_cname(list(range(n)), cn) == 0
        model.set_cname(list(range(n)), cn)
    return impl, model


@pytest.mark.parametrize("n", [8, 70])
@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e"])
def test_received_scenarios(host, name, n):
    X, Y = sessions(n)
    impl, model = fresh(host, n)
    offs = [65530] * n if name == "c" else [(7919 * s) & 0xFFFF for s in range(n)]
    ticks = M.scenario(name, n, 32, 11 + n, Y, offs, walk_max=host.emu_rtcp_sizes(8))
    M.run_received(impl, model, Y, ticks, check)
    if name == "a":                                         # the model's own property: nothing lost, nothing out of order
        for s in range(n):
            blk, _ = model.report_block(s, 1, 0)
            assert blk[4:8] == b"\0\0\0\0" and model.rows[s]["received"] == 64
    if name == "c":
        assert all(r["cycles"] == 65536 for r in model.rows)
    if name == "d":
        assert all(r["bad_seq"] != 65537 or s % 3 == 0 for s, r in enumerate(model.rows))
    if name == "e":
        assert model.rows[3 % n]["received"] > 300
    impl.close()


def test_constant_transit_means_no_jitter(host):
    n = 3
    _, Y = sessions(n)
    impl, model = fresh(host, n)
    for t in range(5):
        items = [(s, t, d, 100 + 2 * t + d, 5000 + Y.ts_offset[s] + t * L) for s in range(n) for d in (0, 1)]
        tick = M.make_tick(items, True, 0)
        M.run_received(impl, model, Y, [tick], check)
    assert all(r["jitter"] == 0 and r["transit"] == 5000 for r in model.rows)
    impl.close()


def test_duplicates_report_fraction_zero_and_the_clamp(host):
    """(b) a negative interval loss reports fraction 0; (f) the cumulative loss is clamped to 24 bits, both ways"""
    n = 4
    X, Y = sessions(n)
    impl, model = fresh(host, n)
    items = [(0, q, 0, 10 + q, 0) for q in range(5)] + [(0, 4, 0, 14, 0)] * 3
    M.run_received(impl, model, Y, [M.make_tick(items, False, 7)], check)
    blk, _ = model.report_block(0, 1, 0)
    assert blk[4] == 0 and blk[5:8] == (-3 & 0xFFFFFF).to_bytes(3, "big")
    w = model.words()
    w[1, :10] = (0, 100, 0x01000000, 65537, 5, 0, 0, 0, 0, 3)              # expected 16777317, 5 received: past 0x7FFFFF
    w[2, :10] = (0, 100, 0, 65537, 0x00900000, 0, 0, 0, 0, 3)              # 101 expected, 9437184 received: below -0x800000
    model.set_words(w)
    impl.set_words(w)
    md, mw = M.both_build(impl, model, X, Y, [0, 1, 2], 99, 1 << 20, check, "clamp")
    blocks = [mw[o + 8 + 4:o + 8 + 8] for o, _ in md]
    assert blocks[1][1:] == b"\x7f\xff\xff" and blocks[1][0] == 255 and blocks[2] == b"\x00\x80\x00\x00"
    impl.close()


@pytest.mark.parametrize("n", [8, 70])
def test_sent_and_build(host, n):
    X, Y = sessions(n)
    X.bound[2] = 0                                          # not bound on the send side: refused
    impl, model = fresh(host, n)
    impl.set_words(model.words())
    model.reset_rows([5])                                   # no CNAME: refused
    impl.lib.emu_rtcp_reset_rows(impl.h, p(np.array([5], np.int32)), 1)
    M.run_received(impl, model, Y, M.scenario("b", n, 4, 3, Y, [5] * n), check)
    Y.bound[n - 1] = 0                                      # no longer bound on the receive side: no block
    M.run_sent_build(impl, model, X, Y, check)
    impl.close()


@pytest.mark.parametrize("n", [8, 70])
def test_loopback(host, n):
    X, Y = sessions(n)
    A, mA = fresh(host, n)
    B, mB = fresh(host, n)
    M.run_received(A, mA, Y, M.scenario("b", n, 3, 1, Y, [9] * n), check)
    M.run_received(B, mB, X, M.scenario("a", n, 3, 2, X, [65000] * n), check)
    rec = np.array([(s, 10 + k, k & 1, 0, 33 + s) for k in range(3) for s in range(n)], np.int32)       # every stream has sent: both sides build SRs
    dg = np.array([(0, 45 + s) for k in range(3) for s in range(n)], np.int32)
    for side, model, sess in ((A, mA, X), (B, mB, Y)):
        assert side.sent(sess, rec, len(rec), dg) == model.sent(rec, len(rec), dg)
    M.run_loopback(A, mA, B, mB, X, Y, check)
    A.close()
    B.close()


def test_order_independence(host):
    """sent and parse: any order of the inputs; received: any interleaving that keeps every stream's own order"""
    import random
    n = 9
    X, Y = sessions(n)
    rng = random.Random(8)
    ticks = M.scenario("b", n, 6, 21, Y, [65500] * n)
    ref, _ = fresh(host, n)
    other, _ = fresh(host, n)
    for tick in ticks:
        ref.received(Y, tick)
        idx = list(range(len(tick["arrivals"])))
        per = [[i for i in idx if tick["arrivals"][i][0] == s] for s in range(n)]
        order = M.interleave(rng, per)
        other.received(Y, dict(arrivals=tick["arrivals"][order].copy(), rtp_seq=tick["rtp_seq"][order].copy(), arrival_time=tick["arrival_time"][order].copy(),
                               now_rtp=tick["now_rtp"]))
        assert np.array_equal(ref.words(), other.words())
    rec, dg = M.random_records(rng, n, 60, 3)
    perm = rng.sample(range(60), 60)
    assert ref.sent(X, rec, 60, dg) == other.sent(X, rec[perm].copy(), 60, dg[perm].copy())
    assert np.array_equal(ref.words(), other.words())
    pkts = [M.write_rr(Y.ssrc[s], [M.write_block(X.ssrc[(s + 1) % n], s, s, s, s, 1 + s, s)]) + M.write_sdes(Y.ssrc[s], b"q") for s in range(n)]
    pkts += [M.write_sr(Y.ssrc[s], s << 32, 0, 0, 0) for s in range(n)] + [M.write_rr(1, []) + M.write_bye([Y.ssrc[3]])]
    offs = np.cumsum([0] + [len(x) for x in pkts])
    wire = np.frombuffer(b"".join(pkts), np.uint8)
    dgr = np.array([(int(offs[k]), len(pkts[k])) for k in range(len(pkts))], np.int32)
    fa, ca = ref.parse(Y, X, dgr, wire, 1 << 40)
    fb, cb = other.parse(Y, X, dgr[rng.sample(range(len(pkts)), len(pkts))].copy(), wire, 1 << 40)
    assert ca == cb and np.array_equal(fa, fb) and np.array_equal(ref.words(), other.words()) and fa[3, 0] & M.BYE_BIT
    ref.close()
    other.close()


def test_argument_rules(host):
    n = 4
    X, Y = sessions(n)
    impl, model = fresh(host, n, names=False)
    lib, h = host, impl.h
    assert lib.emu_rtcp_create(0) is None and lib.emu_rtcp_create(-3) is None
    for streams, names in (([0, 0], [b"a", b"b"]), ([4], [b"a"]), ([-1], [b"a"]), ([0], [b""]), ([0], [b"x" * 32]), ([], [])):
        assert impl.set_cname(streams, names) == -1
    bad = np.frombuffer(b"ab\0c".ljust(32, b"\0"), np.uint8).copy()       # bytes behind the NUL
    assert lib.emu_rtcp_set_cname(h, p(np.array([0], np.int32)), 1, p(bad)) == -1
    assert lib.emu_rtcp_set_cname(h, None, 1, p(bad)) == -1 and lib.emu_rtcp_set_cname(h, p(np.array([0], np.int32)), 1, None) == -1
    assert np.array_equal(impl.words(), model.words())
    assert lib.emu_rtcp_reset_rows(h, p(np.array([1, 1], np.int32)), 2) == -1 and lib.emu_rtcp_reset_rows(h, p(np.array([4], np.int32)), 1) == -1
    arr, seq, cnt, cfg = np.zeros((3, 5), np.int32), np.zeros(3, np.uint16), np.zeros(16, np.int32), Y.cfg()
    rec = lambda *a: lib.emu_rtcp_received(*a)
    assert rec(h, p(cfg), n, L, p(arr), p(seq), 3, None, 0, p(cnt)) == 0
    assert rec(None, p(cfg), n, L, p(arr), p(seq), 3, None, 0, p(cnt)) == -1 and rec(h, None, n, L, p(arr), p(seq), 3, None, 0, p(cnt)) == -1
    assert rec(h, p(cfg), n + 1, L, p(arr), p(seq), 3, None, 0, p(cnt)) == -1 and rec(h, p(cfg), n, L, p(arr), p(seq), -1, None, 0, p(cnt)) == -1
    assert rec(h, p(cfg), n, L, None, p(seq), 3, None, 0, p(cnt)) == -1 and rec(h, p(cfg), n, L, p(arr), None, 3, None, 0, p(cnt)) == -1
    assert rec(h, p(cfg), n, L, p(arr), p(seq), 3, None, 0, None) == -1 and rec(h, p(cfg), n, L, p(arr), p(seq) + 1, 3, None, 0, p(cnt)) == -1
    assert rec(h, p(cfg), n, L, p(arr) + 2, p(seq), 3, None, 0, p(cnt)) == -1 and rec(h, p(cfg), n, L, None, None, 0, None, 0, p(cnt)) == 0
    sc, dg = np.array([3] * 8, np.int32), np.zeros((3, 2), np.int32)
    sent = lambda *a: lib.emu_rtcp_sent(*a)
    assert sent(h, n, p(arr), p(sc), 3, p(dg), p(cnt)) == 0 and sent(h, n, p(arr), p(sc), 0, p(dg), p(cnt)) == -1
    assert sent(h, n - 1, p(arr), p(sc), 3, p(dg), p(cnt)) == -1 and sent(h, n, None, p(sc), 3, p(dg), p(cnt)) == -1
    assert sent(h, n, p(arr), None, 3, p(dg), p(cnt)) == -1 and sent(h, n, p(arr), p(sc), 3, None, p(cnt)) == -1 and sent(h, n, p(arr), p(sc), 3, p(dg), None) == -1
    assert sent(h, n, p(arr), p(sc), 3, p(dg) + 1, p(cnt)) == -1
    idx, wire, cx = np.array([0, 1], np.int32), np.zeros(256, np.uint8), X.cfg()
    cnt64 = np.zeros(8, np.int64)
    bld = lambda *a: lib.emu_rtcp_build(*a)
    ok = (h, p(cx), n, L, p(cfg), n, p(idx), 2, 0, None, p(dg), p(wire), 256, p(cnt64))
    assert bld(*ok) == 0
    for k, v in ((0, None), (1, None), (2, n + 1), (5, n - 1), (6, None), (7, 0), (7, n + 1), (10, None), (11, None), (12, -1), (13, None), (6, p(idx) + 2),
                 (10, p(dg) + 2), (11, p(wire) + 2), (13, p(cnt64) + 4), (9, p(cnt64) + 4)):
        a = list(ok)
        a[k] = v
        assert bld(*a) == -1, k
    fb, tx, ty = np.zeros((n, 8), np.uint32), impl.table(X), impl.table(Y)
    prs = lambda *a: lib.emu_rtcp_parse(*a)
    ok = (h, p(ty), n, p(tx), n, p(dg), 3, p(wire), 256, 0, None, p(fb), p(cnt64))
    assert prs(*ok) == 0
    for k, v in ((0, None), (1, None), (2, n + 1), (4, n + 2), (5, None), (6, -1), (7, None), (8, -1), (11, None), (12, None), (5, p(dg) + 2), (11, p(fb) + 2),
                 (12, p(cnt64) + 4), (10, p(cnt64) + 4)):
        a = list(ok)
        a[k] = v
        assert prs(*a) == -1, k
    a = list(ok)
    a[5], a[6], a[7] = None, 0, None
    assert prs(*a) == 0 and (fb[:, 7] == 0xFFFFFFFF).all()
    impl.close()


def test_standalone_program_builds_and_runs(tmp_path):
    """tests/rtcp_host.cpp is a program of its own with -DRTCP_HOST_MAIN: what a sanitizer build of the host code runs"""
    import subprocess
    from host_build import FLAGS, source
    exe = str(tmp_path / "rtcp_host")
    flags = [f for f in FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.check_call([os.environ.get("CXX", "g++")] + flags + ["-DRTCP_HOST_MAIN", source("rtcp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.startswith("rtcp host ok"), (out.returncode, out.stdout, out.stderr)

"""RTP framing and parsing (solo_rtp_pack / solo_rtp_parse, solo_amd/csrc/solo_rtp.h) without a GPU: the per-record and per-datagram
functions, the three pack passes and the control plane are compiled for the host by this test (tests/rtp_host.cpp, through
tests/host_build.py) and compared with the independent model of tests/rtp_model.py: the parse verdicts in rule order, the timestamp
unwrap at its edges, random records with every refusal reason under both caps, the loopback parse(pack(x)) == x, the binding rules;
then the ABI and the built library's new kernels (no scratch)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import solo_testlib as T
import rtp_model as M
from host_build import host_lib

RTP_SYMBOLS = ("solo_rtp_create", "solo_rtp_destroy", "solo_rtp_bind", "solo_rtp_unbind", "solo_rtp_pack", "solo_rtp_parse")
FILL = 0xA5


@pytest.fixture(scope="module")
def host():
    lib = host_lib("rtp")
    lib.emu_rtp_create.restype = C.c_void_p
    lib.emu_rtp_create.argtypes = [C.c_int, C.c_int]
    lib.emu_rtp_destroy.argtypes = [C.c_void_p]
    lib.emu_rtp_bind.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_int]
    lib.emu_rtp_unbind.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    lib.emu_rtp_table.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    lib.emu_rtp_pack.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                 C.c_longlong, C.c_void_p]
    lib.emu_rtp_parse.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_longlong] + [C.c_void_p] * 4
    return lib


def p(x):
    return None if x is None else x.ctypes.data


class HostSession:
    """the host form's session, bound as the model's session dict says"""

    def __init__(self, lib, ses):
        self.lib, self.ses = lib, ses
        self.h = lib.emu_rtp_create(ses["n_streams"], ses["L"])
        if ses["streams"]:
            assert self.bind(sorted(ses["streams"]), ses["level_id"]) == 0

    def bind(self, streams, level_id, over=None):
        """the listed streams as the session dict has them, or as `over` = {stream: its configuration} says"""
        c = [dict(self.ses["streams"].get(s, {}), **(over or {}).get(s, {})) for s in streams]
        a = [np.array(streams, np.int32), np.array([x["ssrc"] for x in c], np.uint32), np.array([x["ts_offset"] for x in c], np.uint32),
             np.array([x["seq_offset"] for x in c], np.uint16), np.array([x["pt"][0] for x in c], np.uint8), np.array([x["pt"][1] for x in c], np.uint8)]
        return self.lib.emu_rtp_bind(self.h, p(a[0]), len(streams), p(a[1]), p(a[2]), p(a[3]), p(a[4]), p(a[5]), level_id)

    def unbind(self, streams):
        a = np.array(streams, np.int32)
        return self.lib.emu_rtp_unbind(self.h, p(a), len(streams))

    def table(self):
        out = np.zeros(4 + 2 * self.ses["n_streams"], np.uint32)
        assert self.lib.emu_rtp_table(self.h, p(out), out.size) == out.size
        return out

    def pack(self, records, n_records, payload, level=None, max_records=None, cap=None, guard=64):
        records = np.ascontiguousarray(records, np.int32)
        max_records = records.shape[0] if max_records is None else max_records
        cap = 4 * (int(payload.size) + 23 * max_records) if cap is None else cap
        send_count = np.zeros(8, np.int32)
        send_count[0] = n_records
        dg = np.full((max_records + guard, 2), -7, np.int32)
        backing = np.full(cap + guard + 16, FILL, np.uint8)
        a0 = (-backing.ctypes.data) % 4 + 4                           # (a wire that starts at a multiple of 4, with bytes in front of it)
        wire = backing[a0:a0 + cap + guard]
        cnt = np.full(8, -9, np.int32)
        self.lib.emu_rtp_pack(self.h, p(records), p(send_count), max_records, p(payload), payload.size, p(level), 0 if level is None else level.shape[1],
                              p(dg), p(wire), cap, p(cnt))
        if n_records < 0:
            assert cnt[0] == -1 and (cnt[1:] == -9).all() and (dg == -7).all() and (backing == FILL).all()
            return None, None, dict(dgrams=-1)
        c = dict(dgrams=int(cnt[0]), dgrams_needed=int(cnt[1]), bytes=int(cnt[2:4].view(np.int64)[0]), bytes_needed=int(cnt[4:6].view(np.int64)[0]),
                 refused=int(cnt[6]), reserved=int(cnt[7]))
        n = min(n_records, max_records)
        assert (dg[n:] == -7).all() and (wire[cap:] == FILL).all() and (backing[:a0] == FILL).all()      # nothing behind either cap
        assert (wire[c["bytes"]:] == FILL).all()                                                         # ... or behind what was written
        return dg[:n], wire[:c["bytes"]], c

    def parse(self, play, dgrams, wire, want_level=True, want_seq=True):
        dgrams = np.ascontiguousarray(dgrams, np.int32).reshape(-1, 2)
        n = dgrams.shape[0]
        arr = np.full((n + 8, 5), -7, np.int32)
        lv, sq, cnt = np.full(n + 8, 0x77, np.uint8), np.full(n + 8, 0x7777, np.uint16), np.full(8, -9, np.int32)
        play = np.ascontiguousarray(play, np.int32)
        self.lib.emu_rtp_parse(self.h, p(play), p(dgrams), n, p(wire), wire.size, p(arr), p(lv) if want_level else None, p(sq) if want_seq else None, p(cnt))
        assert (arr[n:] == -7).all() and (lv[n:] == 0x77).all() and (sq[n:] == 0x7777).all()
        if not want_level:
            assert (lv == 0x77).all()
        if not want_seq:
            assert (sq == 0x7777).all()
        names = ("accepted", "with_level", "malformed", "version", "unknown_ssrc", "unknown_pt", "timestamp", "reserved")
        return dict(arrivals=arr[:n], level=lv[:n], rtp_seq=sq[:n], count=dict(zip(names, (int(v) for v in cnt))))

    def close(self):
        self.lib.emu_rtp_destroy(self.h)


def lay_out(rng, dgs, front=0, gap=3):
    """datagrams (bytes) -> (dgrams int32 [n,2], wire uint8): back to back at every byte alignment, `front` bytes and random gaps between"""
    wire, table = bytearray(rng.integers(0, 256, front, dtype=np.uint8).tobytes()), []
    for d in dgs:
        wire += rng.integers(0, 256, int(rng.integers(0, gap + 1)), dtype=np.uint8).tobytes()
        table.append((len(wire), len(d)))
        wire += d
    return np.array(table, np.int32).reshape(-1, 2), np.frombuffer(bytes(wire), np.uint8).copy()


def check_parse(got, want):
    assert got["count"] == want["count"], (got["count"], want["count"])
    assert np.array_equal(got["arrivals"], want["arrivals"])
    assert np.array_equal(got["level"], want["level"])
    assert np.array_equal(got["rtp_seq"], want["rtp_seq"])


# ---- structure sizes, ABI -------------------------------------------------------------------------------------------------------------
def test_structure_sizes(host):
    import solo_amd
    assert host.emu_rtp_sizes(0) == 8 == C.sizeof(solo_amd.solo_dgram_t)
    assert host.emu_rtp_sizes(1) == 32 == C.sizeof(solo_amd.solo_rtp_pack_count_t)
    assert host.emu_rtp_sizes(2) == 32 == C.sizeof(solo_amd.solo_rtp_parse_count_t)
    assert host.emu_rtp_sizes(3) == 16
    assert solo_amd.solo_rtp_pack_count_t.bytes.offset == 8 and solo_amd.solo_rtp_pack_count_t.refused.offset == 24
    src = open(os.path.join(T.ROOT, "solo_amd", "csrc", "solo_rtp.h")).read()
    assert 'static_assert(sizeof(SxRtpPackCount) == 32' in src and 'static_assert(sizeof(SxRtpParseCount) == 32' in src


def test_symbols_declared_exported_and_bound():
    import solo_amd
    hdr = T.header_text()
    lib = T.built_library()
    for name in RTP_SYMBOLS:
        assert name in solo_amd.ABI_SYMBOLS and (name + "(") in hdr.replace(" (", "("), name
        assert hasattr(lib, name), name
    bound = solo_amd.load_library()
    assert len(bound.solo_rtp_pack.argtypes) == 13 and len(bound.solo_rtp_parse.argtypes) == 11 and len(bound.solo_rtp_bind.argtypes) == 10
    assert bound.solo_rtp_create.restype is C.c_void_p and bound.solo_rtp_pack.argtypes[5] is C.c_int64 and bound.solo_rtp_parse.argtypes[5] is C.c_int64
    for m in ("bind", "unbind", "pack", "parse", "pack_count", "parse_count", "close"):
        assert callable(getattr(solo_amd.Rtp, m)), m


def test_capture_claims_name_a_test():
    """the header calls solo_rtp_pack and solo_rtp_parse capturable: tests/test_gpu_rtp.py names the test that captures each (its module
    loads without a GPU), as tests/test_gpu_graph_replay.py does for the calls of its table"""
    import ast
    import re
    import test_gpu_rtp as GPU
    m = re.search(r"/\* RTP at both ends.*?\*/", open(os.path.join(T.ROOT, "include", "solo_mi355x.h")).read(), flags=re.S)
    assert m and "captur" in m.group(0) and "solo_rtp_pack" in m.group(0) and "solo_rtp_parse" in m.group(0)
    tests = {n.name for n in ast.parse(open(GPU.__file__).read()).body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}
    assert set(GPU.CAPTURED) == {"solo_rtp_pack", "solo_rtp_parse"} and set(GPU.CAPTURED.values()) <= tests


# ---- the control plane ----------------------------------------------------------------------------------------------------------------
def test_bind_rules(host):
    rng = np.random.default_rng(11)
    ses = M.random_session(rng, 9, 640, 3, unbound=(4,))
    h = HostSession(host, ses)
    t0 = h.table()
    pairs = t0[4:4 + 2 * 8].reshape(8, 2)
    assert t0[0] == 8 and t0[1] == 3 and (np.diff(pairs[:, 0].astype(np.int64)) > 0).all()
    assert {int(a): int(b) for a, b in pairs} == {c["ssrc"]: s for s, c in ses["streams"].items()}
    assert (t0[4 + 16:] == 0).all()
    ok = dict(ssrc=1234567, ts_offset=5, seq_offset=6, pt=(96, 97))
    bad = [([9], 3, {9: ok}), ([-1], 3, {-1: ok}), ([4, 4], 3, {4: ok}), ([], 3, {}), ([4], 15, {4: ok}), ([4], -1, {4: ok}),
           ([4], 3, {4: dict(ok, pt=(128, 97))}), ([4], 3, {4: dict(ok, pt=(96, 255))}),
           ([4], 3, {4: dict(ok, ssrc=ses["streams"][0]["ssrc"])}),                                 # another bound stream's SSRC
           ([4, 5], 3, {4: ok, 5: ok}),                                                             # the same SSRC twice in one call
           ([1], 3, {1: dict(ses["streams"][1], ssrc=ses["streams"][2]["ssrc"])})]                  # a rebind onto a neighbour's
    for streams, level_id, over in bad:
        assert h.bind(streams, level_id, over) == -1, (streams, level_id)
        assert np.array_equal(h.table(), t0), (streams, level_id)                                  # ... and nothing has changed
    # two streams may SWAP their SSRCs in one call; a stream may be bound again with what it has; the latest level id wins
    swap = {1: dict(ses["streams"][1], ssrc=ses["streams"][2]["ssrc"]), 2: dict(ses["streams"][2], ssrc=ses["streams"][1]["ssrc"])}
    assert h.bind([1, 2], 7, swap) == 0
    t1 = h.table()
    assert t1[1] == 7 and {int(a): int(b) for a, b in t1[4:20].reshape(8, 2)}[ses["streams"][2]["ssrc"]] == 1
    assert h.bind([4], 0, {4: ok}) == 0 and h.table()[0] == 9 and h.table()[1] == 0
    assert h.unbind([4, 0]) == 0 and h.table()[0] == 7
    assert h.unbind([4]) == 0 and h.table()[0] == 7     # (not bound: stays so)
    for lst in ([9], [0, 0], []):
        assert h.unbind(lst) == -1
    assert h.bind([0], 2, {0: dict(ok, ssrc=ses["streams"][0]["ssrc"])}) == 0                    # a freed SSRC can be bound again
    h.close()


# ---- parse: the verdicts ----------------------------------------------------------------------------------------------------------------
def test_model_gives_the_hostile_kinds_their_stated_verdicts():
    rng = np.random.default_rng(5)
    ses = M.random_session(rng, 6, 640, 5)
    play = rng.integers(0, 5000, 6)
    kinds = M.hostile_kinds(ses, play, 2, rng)
    names = [k[0] for k in kinds]
    for must in ("cc1", "cc15", "padding", "level_after_others", "level_len2", "overrun", "other_profile", "x_no_room", "version1", "truncated_11", "zero_payload"):
        assert must in names
    dg, wire = lay_out(rng, [k[1] for k in kinds], front=1)
    got = M.model_parse(ses, play, dg, wire)
    for (name, _, verdict, level), v, lv, a in zip(kinds, got["verdicts"], got["level"], got["arrivals"]):
        assert v == verdict, (name, v)
        if verdict == "accepted":
            assert lv == level and a[0] == 2, (name, lv)
        else:
            assert tuple(a) == M.REJECTED and lv == 255
    assert set(got["verdicts"]) == set(M.VERDICTS)


@pytest.mark.parametrize("L", [640, 320, 1280])
def test_parse_verdicts_in_rule_order(host, L):
    rng = np.random.default_rng(100 + L)
    ses = M.random_session(rng, 6, L, 5, unbound=(3,), equal_pt=(1,))
    play = rng.integers(0, 5000, 6).astype(np.int32)
    h = HostSession(host, ses)
    kinds = M.hostile_kinds(ses, play, 2, rng) + M.hostile_kinds(ses, play, 5, rng)
    c1 = ses["streams"][1]
    kinds.append(("equal_pt", M.build(c1["ssrc"], 98, 1, c1["ts_offset"] + int(play[1]) * L, b"xyz"), "accepted", 255))
    order = rng.permutation(len(kinds))
    dg, wire = lay_out(rng, [kinds[i][1] for i in order], front=5)
    want = M.model_parse(ses, play, dg, wire)
    assert [kinds[i][2] for i in order] == want["verdicts"]
    check_parse(h.parse(play, dg, wire), want)
    eq = list(order).index(len(kinds) - 1)
    assert want["arrivals"][eq, 0] == 1 and want["arrivals"][eq, 2] == -1 and want["arrivals"][eq, 4] == 3
    # datagram ranges that leave the wire: malformed, never read
    good = want["verdicts"].index("accepted")
    out = np.array([[-1, 40], [wire.size - 39, 40], [wire.size, 12], [2 ** 31 - 1, 2 ** 31 - 1], [0, -5], [dg[good, 0], dg[good, 1]]], np.int32)
    want = M.model_parse(ses, play, out, wire)
    assert want["count"]["malformed"] == 5 and want["count"]["accepted"] == 1
    check_parse(h.parse(play, out, wire), want)
    # both optional outputs absent; no datagram at all
    got = h.parse(play, dg, wire, want_level=False, want_seq=False)
    assert got["count"] == M.model_parse(ses, play, dg, wire)["count"]
    assert h.parse(play, dg[:0], wire)["count"]["accepted"] == 0
    # without a level id nothing carries a level
    assert h.bind([0], 0) == 0
    ses0 = dict(ses, level_id=0)
    want = M.model_parse(ses0, play, dg, wire)
    assert want["count"]["with_level"] == 0 and (want["level"] == 255).all() and want["count"]["accepted"] > 0
    check_parse(h.parse(play, dg, wire), want)
    h.close()


def test_unwrap_rule_at_its_edges(host):
    L = 640
    ses = M.session(4, L, 0, {0: dict(ssrc=10, ts_offset=0xFFFFFF00, seq_offset=0xFFFE, pt=(96, 97)), 1: dict(ssrc=11, ts_offset=0, seq_offset=0, pt=(96, 97)),
                              2: dict(ssrc=12, ts_offset=0x80000000, seq_offset=1, pt=(96, 97))})
    h = HostSession(host, ses)
    rng = np.random.default_rng(9)
    cases = []           # (stream, play, timestamp on the wire, expected seq or None)

    def ts_of(stream, seq):
        return (ses["streams"][stream]["ts_offset"] + seq * L) % 2 ** 32

    for stream in (0, 1, 2):
        for play in (0, 1, 6710885, 6710886, 6710887, 6710888, 2 * 6710886, 2 * 6710886 + 1, 10 ** 9, M.INT32_MAX - 1, M.INT32_MAX):
            for d in (-2, -1, 0, 1, 2, 4095):
                seq = play + d
                cases.append((stream, play, ts_of(stream, seq), seq if 0 <= seq <= M.INT32_MAX else None))     # (below 0 / above 2^31 - 1: refused)
            cases.append((stream, play, ts_of(stream, play) + 1, None))                                         # delta not a multiple of L
            cases.append((stream, play, ts_of(stream, play + 1) - 1, None))
            cases.append((stream, play, ts_of(stream, play) + L // 2, None))
    assert 6710886 * L < 2 ** 32 < 6710887 * L
    assert any(c[3] is None and c[1] == 0 for c in cases) and any(c[3] is None and c[1] == M.INT32_MAX for c in cases)
    for stream, play, ts, seq in cases:
        d = M.build(ses["streams"][stream]["ssrc"], 96, 0, ts, b"\x01\x02")
        dg, wire = lay_out(rng, [d], front=int(rng.integers(0, 4)))
        pl = np.zeros(4, np.int32)
        pl[stream] = play
        got, want = h.parse(pl, dg, wire), M.model_parse(ses, pl, dg, wire)
        check_parse(got, want)
        if seq is None:
            assert got["count"]["timestamp"] == 1 and tuple(got["arrivals"][0]) == M.REJECTED, (stream, play, ts)
        else:
            assert got["count"]["accepted"] == 1 and tuple(got["arrivals"][0][:3]) == (stream, seq, 0), (stream, play, ts, got["arrivals"][0])
    # the far ends of the window: +-(2^31 / L) packets around the play-out position
    half = 2 ** 31 // L
    for d, ok in ((half - 1, True), (-half, True), (half + 1, False), (-half - 2, False)):
        play = 2 * 10 ** 8 + 7 * half
        pl = np.array([0, play, 0, 0], np.int32)
        dg, wire = lay_out(rng, [M.build(11, 97, 0, ts_of(1, play + d), b"q")])
        got = h.parse(pl, dg, wire)
        check_parse(got, M.model_parse(ses, pl, dg, wire))
        assert (got["arrivals"][0, 1] == play + d) == ok                     # (outside the window a packet lands elsewhere: the ring's window sorts it out)
    # the 16-bit sequence number wraps inside the run: seq_offset 0xFFFE, packets 0 .. 2, both descriptions
    rec = np.array([[0, s, d, 4 * s, 3] for s in range(3) for d in (0, 1)], np.int32)
    pool = np.arange(64, dtype=np.uint8)
    dg, wire, cnt = h.pack(rec, 6, pool)
    assert cnt["dgrams"] == 6 and cnt["refused"] == 0
    got = h.parse(np.zeros(4, np.int32), dg, wire)
    assert list(got["rtp_seq"]) == [0xFFFE, 0xFFFF, 0, 1, 2, 3]
    assert np.array_equal(got["arrivals"][:, :3], rec[:, :3])
    # ... and the timestamp with it: ts_offset 0xFFFFFF00 + 640 wraps at packet 1
    assert [int.from_bytes(bytes(wire[o + 4:o + 8]), "big") for o in dg[:, 0]] == [0xFFFFFF00, 0xFFFFFF00, 0x180, 0x180, 0x400, 0x400]
    h.close()


# ---- pack against the model -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_level", [False, True])
def test_host_pack_against_model(host, with_level):
    rng = np.random.default_rng(2000 + with_level)
    ses = M.random_session(rng, 12, 640, 9, unbound=(3, 8), equal_pt=(5,))
    h = HostSession(host, ses)
    n, pool_bytes, depth = 700, 5003, 7                            # three tiles, the last one partly filled
    backing = rng.integers(0, 256, pool_bytes + 3, dtype=np.uint8)
    pool = backing[1:1 + pool_bytes]                               # (a pool at an odd address)
    rec = M.random_records(rng, ses, n, pool_bytes, seq_hi=2 ** 31)
    rec[::50, 1] = M.INT32_MAX
    level = rng.integers(0, 256, (12, depth), dtype=np.uint8) if with_level else None
    full = M.model_pack(ses, rec, n, pool, level)
    assert all(full["reasons"].get(r, 0) > 0 for r in ("stream", "unbound", "desc", "seq", "len", "long", "range")), full["reasons"]
    assert len({(int(a), int(b)) for a, b in rec[:, 3:5]}) < n       # offsets do repeat
    alld = full["all_dgrams"]
    need_b = full["count"]["bytes_needed"]
    assert full["count"]["dgrams_needed"] > 400 and need_b == alld[alld[:, 1] > 0][-1].sum() + (-alld[alld[:, 1] > 0][-1].sum()) % 4
    valid = np.nonzero(alld[:, 1] > 0)[0]
    k = int(valid[len(valid) // 2])
    k_odd = int(next(v for v in valid[300:] if alld[v, 1] % 4))    # a datagram with pad bytes behind it
    end_odd = int(alld[k_odd, 0] + alld[k_odd, 1])
    # the caps: none; exactly what is needed; a datagram boundary; a byte short of one; inside a header; between a datagram's end and its
    # pad bytes (it is then not written); zero; and the record count cut by max_records and by the sender's count
    for n_rec, max_records, cap in [(n, n, None), (n, n, need_b), (n, n, int(alld[k, 0])), (n, n, int(alld[k, 0] + alld[k, 1] - 1)), (n, n, int(alld[k, 0] + 5)),
                                    (n, n, end_odd), (n, n, (end_odd + 3) & ~3), (n, n, 0), (n, n, 3), (n, 300, None), (256, n, None), (257, n, None), (0, n, None),
                                    (n + 50, n, None), (n, 1, None), (-1, n, None), (-2 ** 31, n, 100)]:
        want = M.model_pack(ses, rec, n_rec, pool, level, max_records, cap)
        dg, wire, cnt = h.pack(rec, n_rec, pool, level, max_records, cap)
        assert cnt == want["count"], (n_rec, max_records, cap, cnt, want["count"])
        if n_rec >= 0:
            assert np.array_equal(dg, want["dgrams"]), (n_rec, max_records, cap)
            assert np.array_equal(wire, want["wire"]), (n_rec, max_records, cap)
    want = M.model_pack(ses, rec, n, pool, level, n, end_odd)
    assert want["dgrams"][k_odd, 1] == 0 and want["count"]["dgrams"] == int((valid < k_odd).sum())
    h.close()


def test_host_pack_fanout_shape(host):
    """8 destinations share 2 sources' offsets: the wire holds every destination's copy under its own header"""
    rng = np.random.default_rng(31)
    ses = M.random_session(rng, 8, 640, 0)
    h = HostSession(host, ses)
    pool = rng.integers(0, 256, 300, dtype=np.uint8)
    src = [(0, 41), (41, 33), (74, 50), (124, 29)]                 # (source, description) -> (offset, len)
    rec = np.array([[d, 100 + pk, desc, src[2 * (d % 2) + desc][0] + 150 * pk * 0, src[2 * (d % 2) + desc][1]] for pk in range(2) for d in range(8) for desc in (0, 1)],
                   np.int32)
    want = M.model_pack(ses, rec, 32, pool)
    dg, wire, cnt = h.pack(rec, 32, pool)
    assert cnt == want["count"] and cnt["dgrams"] == 32 and cnt["bytes"] > 4 * 300
    assert np.array_equal(dg, want["dgrams"]) and np.array_equal(wire, want["wire"])
    h.close()


# ---- loopback -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_level", [False, True])
def test_loopback_parse_of_pack(host, with_level):
    rng = np.random.default_rng(300 + with_level)
    ses = M.random_session(rng, 10, 1280, 14, equal_pt=(2, 7))
    h = HostSession(host, ses)
    n, pool_bytes, depth = 600, 4001, 5
    pool = rng.integers(0, 256, pool_bytes, dtype=np.uint8)
    play = rng.integers(0, 2 ** 31 - 4000, 10).astype(np.int32)
    rec = M.random_records(rng, ses, n, pool_bytes, hostile=False)
    rec[:, 1] = play[rec[:, 0]] + rng.integers(-3, 4000, n)
    rec[:, 1] = np.maximum(rec[:, 1], 0)
    level = rng.integers(0, 255, (10, depth), dtype=np.uint8) if with_level else None      # (255 reads back as "no level")
    dg, wire, cnt = h.pack(rec, n, pool, level)
    assert cnt["dgrams"] == n and cnt["refused"] == 0
    H = 20 if with_level else 12
    got = h.parse(play, dg, wire)
    check_parse(got, M.model_parse(ses, play, dg, wire))
    a = got["arrivals"]
    eq = np.isin(rec[:, 0], (2, 7))
    assert got["count"]["accepted"] == n and got["count"]["with_level"] == (n if with_level else 0)
    assert np.array_equal(a[:, 0], rec[:, 0]) and np.array_equal(a[:, 1], rec[:, 1]) and np.array_equal(a[:, 4], rec[:, 4])
    assert np.array_equal(a[:, 2], np.where(eq, -1, rec[:, 2]))
    assert np.array_equal(a[:, 3], dg[:, 0] + H) and np.array_equal(dg[:, 1], rec[:, 4] + H) and (dg[:, 0] % 4 == 0).all()
    for k in range(n):
        assert np.array_equal(wire[a[k, 3]:a[k, 3] + a[k, 4]], pool[rec[k, 3]:rec[k, 3] + rec[k, 4]]), k
    so = np.array([ses["streams"][int(s)]["seq_offset"] for s in rec[:, 0]], np.int64)
    assert np.array_equal(got["rtp_seq"], ((so + 2 * rec[:, 1].astype(np.int64) + rec[:, 2]) % 65536).astype(np.uint16))
    if with_level:
        assert np.array_equal(got["level"], level[rec[:, 0], rec[:, 1] % depth])
    else:
        assert (got["level"] == 255).all()
    h.close()


# ---- the Python binding refuses bad arguments before the library ------------------------------------------------------------------------
def test_binding_checks():
    import solo_amd
    torch = pytest.importorskip("torch")
    o = object.__new__(solo_amd.Rtp)
    o.n_rows = o.n_streams = 8
    o.packet_samples, o.level_id = 640, 3
    o.torch, o.lib, o.h, o.device = torch, T.NoLib(), None, torch.device("cpu")
    o._stream = lambda: None
    ok = dict(streams=[1, 2], ssrc=[5, 6])
    for over in (dict(streams=[1, 1]), dict(streams=[8]), dict(streams=[]), dict(ssrc=[5]), dict(ssrc=[5, 2 ** 32]), dict(ssrc=-1), dict(ts_offset=2 ** 32),
                 dict(seq_offset=65536), dict(pt=(96, 128)), dict(pt=(96,)), dict(pt=[(96, 97)]), dict(level_id=15), dict(level_id=-1)):
        with pytest.raises(ValueError):
            o.bind(**dict(ok, **over))
    for lst in ([], [8], [0, 0]):
        with pytest.raises(ValueError):
            o.unbind(lst)
        with pytest.raises(ValueError):
            o.reset(lst)

    class Recorder:
        calls = []

        def __getattr__(self, name):
            return lambda *a: self.calls.append((name,) + tuple(tuple(x) if isinstance(x, C.Array) else x for x in a)) or 0
    o.lib, o.h = Recorder(), 0x77
    o.reset()                                                     # reset() of the row objects, here: unbind every stream / the listed ones
    o.reset([5, 2])
    assert Recorder.calls == [("solo_rtp_unbind", 0x77, tuple(range(8)), 8, None), ("solo_rtp_unbind", 0x77, (5, 2), 2, None)]
    o.lib, o.h = T.NoLib(), None
    D = T.FakeDev
    I32, U8, I16 = torch.int32, torch.uint8, torch.int16
    good = dict(records=D((10, 5), I32), send_count=D((8,), I32), payload=D((100,), U8), level=D((8, 4), U8), dgrams=D((10, 2), I32), wire=D((999,), U8))
    for over in (dict(records=D((10, 4), I32)), dict(records=D((10, 5), I32, cuda=False)), dict(records=D((0, 5), I32)), dict(send_count=D((6,), I32)),
                 dict(send_count=None), dict(payload=D((100,), I32)), dict(level=D((7, 4), U8)), dict(level=D((8, 0), U8)), dict(dgrams=D((9, 2), I32)),
                 dict(wire=D((999,), U8, contiguous=False)), dict(wire=D((9, 9), U8))):
        with pytest.raises(ValueError):
            o.pack(**dict(good, **over))
    o.level_id = 0
    with pytest.raises(ValueError):
        o.pack(**good)                                            # levels without a level id
    b = object.__new__(solo_amd.SoloBatch)
    b.n_streams, b.packet_samples, b.h = 8, 640, None
    good = dict(batch=b, dgrams=D((10, 2), I32), wire=D((999,), U8), arrivals=D((10, 5), I32), level=D((10,), U8), rtp_seq=D((10,), I16))
    b2 = object.__new__(solo_amd.SoloBatch)
    b2.n_streams, b2.packet_samples, b2.h = 8, 1280, None
    for over in (dict(batch=None), dict(batch=b2), dict(dgrams=D((10, 3), I32)), dict(wire=D((999,), I16)), dict(arrivals=D((9, 5), I32)), dict(level=D((9,), U8)),
                 dict(rtp_seq=D((10,), U8)), dict(rtp_seq=D((10,), I16, cuda=False))):
        with pytest.raises(ValueError):
            o.parse(**dict(good, **over))


# ---- the built library's kernels ------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="no LLVM binutils on this box")
def test_rtp_kernels_use_no_scratch():
    import solo_amd
    T.built_library()
    sys.path.insert(0, os.path.join(T.ROOT, "tools"))
    from kernel_resources import kernel_resources
    seen = kernel_resources(solo_amd.LIB_PATH)
    for frag in ("solo_rtp_totals_kernel", "solo_rtp_scan_kernel", "solo_rtp_scatter_kernel", "solo_rtp_parse_kernel", "solo_rtp_clear_kernel", "solo_rtp_bind_kernel"):
        hits = [r for name, r in seen.items() if frag in name]
        assert len(hits) == 1, (frag, len(hits))                  # rate-independent: compiled once
        assert hits[0]["scratch"] == 0, (frag, hits[0])

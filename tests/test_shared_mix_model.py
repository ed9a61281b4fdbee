"""Shared listener mixes without a GPU (solo_mix_shared, solo_send_fanout): the passes of solo_amd/csrc/solo_mix_shared.h and
solo_fanout.h are compiled for the host by this test (tests/shared_mix_host.cpp, through tests/host_build.py) and compared bit
for bit with the independent model of tests/shared_mix_model.py -- PCM, lists, source table, counts, records, pool bytes, and the fill
behind the counts."""
import ctypes as C

import numpy as np
import pytest

from host_build import host_lib
from mix_model import model_mix, ties_decide
from shared_mix_model import fanout_case, heard, model_fanout, model_mix_shared, shared_case

FILL = dict(pcm_spk=0x1234, spk_list=-7001, spk_rows=-7002, pcm_room=0x4321, room_list=-7003, source=-7004, energy=-77, mixed=0xA5)
DTYPE = dict(pcm_spk=np.int16, spk_list=np.int32, spk_rows=np.int32, pcm_room=np.int16, room_list=np.int32, source=np.int32, energy=np.int64,
             mixed=np.uint8)
FILL_C = 0x5A5A5A5A
MIX_COUNT = ("rows", "rooms", "speakers", "shared")
SEND_COUNT = ("records", "records_needed", "bytes", "bytes_needed", "empty", "refused")


@pytest.fixture(scope="module")
def host():
    lib = host_lib("shared_mix")
    V, I = C.c_void_p, C.c_int
    lib.emu_mix_shared.argtypes = [V, I, I, I, V, I, V, I, V, V, V, V, V, V, V, V, V, V, V]
    lib.emu_send_fanout.argtypes = [V, V, I, V, V, I, V, I, I, I, V, I, V, I, V, C.c_longlong, V]
    return lib


def aligned(shape, dtype, fill=0):
    """an array whose first byte is 16-byte aligned (the interface's rule for PCM)"""
    nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
    raw = np.zeros(nbytes + 16, np.uint8)
    off = (-raw.ctypes.data) % 16
    a = raw[off:off + nbytes].view(dtype).reshape(shape)
    a[...] = fill
    return a


def ptr(a):
    return a.ctypes.data if a is not None else None


def mix_buffers(n, n_rooms, P, L):
    shapes = dict(pcm_spk=(n, P, L), spk_list=(n,), spk_rows=(n,), pcm_room=(n_rooms, P, L), room_list=(n_rooms,), source=(n,), energy=(n, P),
                  mixed=(n, P))
    b = {k: aligned(s, DTYPE[k], FILL[k]) for k, s in shapes.items()}
    b["count"] = np.full(6, FILL_C, np.int32)
    return b


def mix_count(cnt):
    c = {k: int(cnt[i]) for i, k in enumerate(MIX_COUNT)}
    c["clipped"] = int(cnt[4:6].view(np.int64)[0])
    return c


def run_mix(host, pcm, room, n_rooms, gain, K, keep, slots, drop=()):
    n, P, L = pcm.shape
    x = aligned(pcm.shape, np.int16)
    x[...] = pcm
    b = mix_buffers(n, n_rooms, P, L)
    room = np.ascontiguousarray(room, np.int32)
    a = {k: (None if k in drop else v) for k, v in b.items()}
    ret = host.emu_mix_shared(ptr(x), n, P, L, ptr(room), n_rooms, ptr(gain), K, ptr(keep), ptr(slots), ptr(a["pcm_spk"]), ptr(a["spk_list"]),
                              ptr(a["spk_rows"]), ptr(a["pcm_room"]), ptr(a["room_list"]), ptr(a["source"]), ptr(a["energy"]), ptr(a["mixed"]),
                              ptr(a["count"]))
    return ret, b


def mix_want(pcm, room, n_rooms, gain, K, keep, slots):
    n, P, L = pcm.shape
    return model_mix_shared(pcm, room, n_rooms, gain, K, keep, slots, fill={k: v for k, v in mix_buffers(n, n_rooms, P, L).items() if k != "count"})


def same(got, want, skip=()):
    """every array against the model (which started from the same fill: what must not be written is compared too)"""
    for k in FILL:
        if k not in skip:
            bad = np.argwhere(got[k] != want[k])
            assert len(bad) == 0, (k, bad[:6].tolist())


@pytest.mark.parametrize("L,P,K", [(320, 1, 3), (320, 3, 3), (640, 1, 3), (640, 3, 3), (1280, 1, 3), (1280, 3, 3), (640, 3, 1), (640, 3, 2), (640, 3, 64)])
def test_host_mix_shared_against_model(host, L, P, K):
    pcm, room, gain, n_rooms, keep, slots, marks = shared_case(300 + L + P + K, P, L, K)
    n = len(room)
    sizes = set(np.bincount(room[room >= 0]).tolist())
    assert {1, 2, K, K + 1, 9, 70} <= sizes and (room < 0).sum() >= 6 and (np.diff(slots) > 1).any() and {0, -5, 32767} <= set(gain.tolist())
    want = mix_want(pcm, room, n_rooms, gain, K, keep, slots)
    c = want["count"]
    # the case has what it was built for
    assert c["clipped"] > 0 and 0 < c["shared"] < c["rooms"] and 0 < c["speakers"] < c["rows"] == (room >= 0).sum()
    assert ties_decide(want["energy"], room, K) > 0
    assert want["source"][marks["silent"]] < n                                                       # a speaker ...
    if K <= 3:
        assert not want["mixed"][marks["silent"]].any()                                              # ... only because it is kept
    assert marks["kept_room"] not in want["room_list"][:c["shared"]].tolist()                        # a room of speakers only
    assert want["source"][marks["loose_kept"]] == -1
    if K == 3 and P == 3:
        assert want["mixed"][marks["once"]].tolist() == [1, 0, 0] and not keep[marks["once"]]        # a speaker in packet 0 only
    # ... and the model agrees with the model of solo_mix on what everybody hears
    ref = model_mix(pcm, room, n_rooms, gain, K)
    assert np.array_equal(heard(want, n)[room >= 0], ref["out"][room >= 0])
    ret, got = run_mix(host, pcm, room, n_rooms, gain, K, keep, slots)
    assert ret == 0 and mix_count(got["count"]) == c, (mix_count(got["count"]), c)
    same(got, want)


def test_host_mix_shared_without_the_optional_arguments(host):
    P, L, K = 2, 640, 3
    pcm, room, gain, n_rooms, keep, slots, marks = shared_case(11, P, L, K, big=20)
    want = mix_want(pcm, room, n_rooms, None, K, None, None)
    ret, got = run_mix(host, pcm, room, n_rooms, None, K, None, None, drop=("spk_rows", "energy", "mixed"))
    assert ret == 0 and mix_count(got["count"]) == want["count"]
    same(got, want, skip=("spk_rows", "energy", "mixed"))
    assert (got["spk_rows"] == FILL["spk_rows"]).all() and (got["energy"] == FILL["energy"]).all() and (got["mixed"] == FILL["mixed"]).all()
    assert np.array_equal(want["spk_list"][:want["count"]["speakers"]], want["spk_rows"][:want["count"]["speakers"]])


def _untouched(b, count_from=1):
    return all((b[k] == FILL[k]).all() for k in FILL) and (b["count"][count_from:] == FILL_C).all()


def test_mix_shared_host_refusals(host):
    P, L, K = 2, 320, 3
    pcm, room, gain, n_rooms, keep, slots, _ = shared_case(12, P, L, K, big=12)
    n = len(room)
    x = aligned(pcm.shape, np.int16)
    x[...] = pcm
    b = mix_buffers(n + 1, n_rooms + 1, P, L)
    room = np.ascontiguousarray(room, np.int32)
    row = P * L * 2

    def call(pin=ptr(x), n=n, P=P, L=L, room=ptr(room), n_rooms=n_rooms, K=K, spk=ptr(b["pcm_spk"]), spk_list=ptr(b["spk_list"]),
             proom=ptr(b["pcm_room"]), room_list=ptr(b["room_list"]), source=ptr(b["source"]), count=ptr(b["count"])):
        return host.emu_mix_shared(pin, n, P, L, room, n_rooms, ptr(gain), K, ptr(keep), ptr(slots), spk, spk_list, ptr(b["spk_rows"]), proom,
                                   room_list, source, ptr(b["energy"]), ptr(b["mixed"]), count)

    # what solo_mix refuses
    assert call(pin=None) == -1 and call(room=None) == -1
    assert call(n=0) == -1 and call(n=-3) == -1 and call(P=0) == -1 and call(n_rooms=0) == -1 and call(n_rooms=n + 1) == -1
    assert call(n=2, P=2 ** 30, n_rooms=1) == -1                                       # n * n_packets = 2^31
    assert call(pin=ptr(x) + 2) == -1 and call(spk=ptr(b["pcm_spk"]) + 8) == -1 and call(proom=ptr(b["pcm_room"]) + 4) == -1      # not 16-byte aligned
    # max_speakers outside [1, 64]
    assert call(K=0) == -1 and call(K=-1) == -1 and call(K=65) == -1
    # required outputs
    assert call(spk=None) == -1 and call(spk_list=None) == -1 and call(proom=None) == -1 and call(room_list=None) == -1
    assert call(source=None) == -1 and call(count=None) == -1
    # overlaps: each output with the input, and the outputs with each other (by one row at either end)
    assert call(spk=ptr(x)) == -1 and call(proom=ptr(x)) == -1 and call(proom=ptr(b["pcm_spk"])) == -1
    assert call(spk=ptr(x) + (n - 1) * row) == -1 and call(pin=ptr(b["pcm_spk"]) + (n - 1) * row) == -1
    assert call(proom=ptr(x) + (n - 1) * row) == -1 and call(pin=ptr(b["pcm_room"]) + (n_rooms - 1) * row) == -1
    assert call(proom=ptr(b["pcm_spk"]) + (n - 1) * row) == -1 and call(spk=ptr(b["pcm_room"]) + (n_rooms - 1) * row) == -1
    assert _untouched(b, 0)
    assert call() == 0 and b["count"][0] == (room >= 0).sum()


@pytest.mark.parametrize("what", ["room_low", "room_high", "room_max", "slots_negative", "slots_equal", "slots_falling"])
def test_mix_shared_device_refusals(host, what):
    P, L, K = 2, 320, 3
    pcm, room, gain, n_rooms, keep, slots, _ = shared_case(13, P, L, K, big=12)
    room, slots = room.copy(), slots.copy()
    if what.startswith("room"):
        room[5] = dict(room_low=-2, room_high=n_rooms, room_max=2 ** 31 - 1)[what]
    elif what == "slots_negative":
        slots[0] = -1
    else:
        slots[9] = slots[8] if what == "slots_equal" else slots[8] - 1
    ret, got = run_mix(host, pcm, room, n_rooms, gain, K, keep, slots)
    assert ret == -2 and got["count"][0] == -1 and _untouched(got)
    assert model_mix_shared(pcm, room, n_rooms, gain, K, keep, slots)["count"]["rows"] == -1


# ---- solo_send_fanout ------------------------------------------------------------------------------------------------------------------
R_FILL, P_FILL = -9, 0xEE
SLOT, HBB = 96, 8


def run_fan(host, case, max_records, cap, first_seq=500, with_optional=True, guard=4):
    bits, nbytes, source, dst_stream, send, seq_base = case
    n_src, P, slot = bits.shape
    n_dst = len(source)
    rec = np.full((max_records + guard, 5), R_FILL, np.int32)
    pay = np.full(cap + guard, P_FILL, np.uint8)
    cnt = np.full(8, FILL_C, np.int32)
    keepalive = [np.ascontiguousarray(a) for a in (dst_stream, send, seq_base)]
    ret = host.emu_send_fanout(ptr(bits), ptr(nbytes), n_src, ptr(source), ptr(keepalive[0]) if with_optional else None, n_dst,
                               ptr(keepalive[1]) if with_optional else None, P, slot, HBB, ptr(keepalive[2]) if with_optional else None, first_seq,
                               ptr(rec), max_records, ptr(pay), cap, ptr(cnt))
    return ret, rec, pay, cnt


def send_count(cnt):
    v = cnt.view(np.int32)
    return dict(records=int(v[0]), records_needed=int(v[1]), bytes=int(v[2:4].view(np.int64)[0]), bytes_needed=int(v[4:6].view(np.int64)[0]), empty=int(v[6]),
                refused=int(v[7]))


def fan_want(case, max_records, cap, first_seq=500, with_optional=True, guard=4):
    bits, nbytes, source, dst_stream, send, seq_base = case
    o = dict(dst_stream=dst_stream, send=send, seq_base=seq_base) if with_optional else {}
    return model_fanout(bits, nbytes, source, HBB, first_seq=first_seq, max_records=max_records, cap=cap,
                        records=np.full((max_records + guard, 5), R_FILL, np.int32), payload=np.full(cap + guard, P_FILL, np.uint8), **o)


@pytest.fixture(scope="module")
def fan_case():
    return fanout_case(21, 10, 20, 5, SLOT, HBB)


def test_fanout_case_has_everything(fan_case):
    bits, nbytes, source, dst_stream, send, seq_base = fan_case
    w = fan_want(fan_case, 2 * 20 * 5, 10 * 5 * SLOT)
    c, rec = w["count"], w["all_records"]
    assert c["empty"] >= 5 and c["refused"] >= 4 and c["records"] == c["records_needed"] > 40 and c["bytes"] == c["bytes_needed"] > 0
    assert (nbytes[0].view(np.uint8) == 0xA5).all() and set(np.unique(send & 3)) == {0, 1, 2, 3} and (source == -1).sum() >= 2
    assert (source == 4).sum() >= 3
    offs = rec[:, 3]
    assert len(set(offs.tolist())) < len(offs)                                           # destinations of one source share their datagrams
    assert c["bytes_needed"] < int(rec[:, 4].sum())                                      # ... which the pool holds once
    # a datagram nobody sends (every destination of its source masks it) is in the pool all the same
    held = {(int(o), int(l)) for o, l in rec[:, 3:5]}
    assert sum(l for _, l in held) < c["bytes_needed"]


def test_host_fanout_against_model(host, fan_case):
    full_r, full_b = 2 * 20 * 5, 10 * 5 * SLOT
    w = fan_want(fan_case, full_r, full_b)
    need_r, need_b = w["count"]["records_needed"], w["count"]["bytes_needed"]
    tick_r = int((w["all_records"][:, 1] - np.asarray(fan_case[5])[np.searchsorted(fan_case[3], w["all_records"][:, 0])] - 500 < 2).sum())
    caps = [(full_r, full_b), (need_r, need_b), (need_r - 1, need_b - 1), (tick_r + 3, full_b), (full_r, need_b * 2 // 5 + 1), (tick_r - 2, need_b // 2),
            (0, full_b), (full_r, 0), (0, 0)]
    seen = set()
    for max_records, cap in caps:
        want = fan_want(fan_case, max_records, cap)
        ret, rec, pay, cnt = run_fan(host, fan_case, max_records, cap)
        assert ret == 0 and send_count(cnt) == want["count"], (max_records, cap, send_count(cnt), want["count"])
        assert np.array_equal(rec, want["records"]) and np.array_equal(pay, want["payload"]), (max_records, cap)
        c = want["count"]
        seen.add((c["records"] < c["records_needed"], c["bytes"] < c["bytes_needed"]))
        assert c["records_needed"] == need_r and c["bytes_needed"] == need_b and c["records"] <= max_records and c["bytes"] <= cap
    assert seen == {(False, False), (True, False), (True, True)}
    # without stream numbers, masks and sequence bases
    want = fan_want(fan_case, full_r, full_b, with_optional=False)
    ret, rec, pay, cnt = run_fan(host, fan_case, full_r, full_b, with_optional=False)
    assert ret == 0 and send_count(cnt) == want["count"] and np.array_equal(rec, want["records"]) and np.array_equal(pay, want["payload"])
    # sequence numbers that leave int32: those packets are refused, per destination
    want = fan_want(fan_case, full_r, full_b, first_seq=2 ** 31 - 300)
    ret, rec, pay, cnt = run_fan(host, fan_case, full_r, full_b, first_seq=2 ** 31 - 300)
    assert want["count"]["refused"] > w["count"]["refused"] and 0 < want["count"]["records"] < need_r
    assert ret == 0 and send_count(cnt) == want["count"] and np.array_equal(rec, want["records"]) and np.array_equal(pay, want["payload"])


def test_unnamed_rows_do_not_count(host, fan_case):
    """whatever the length records (and the bytes) of rows nobody names hold, the output is the same"""
    bits, nbytes, source, dst_stream, send, seq_base = fan_case
    full_r, full_b = 2 * 20 * 5, 10 * 5 * SLOT
    ret, rec, pay, cnt = run_fan(host, fan_case, full_r, full_b)
    unnamed = sorted(set(range(10)) - set(source.tolist()))
    assert {0, 1} <= set(unnamed)
    nb2, bits2 = nbytes.copy(), bits.copy()
    nb2[unnamed] = (40, 20)
    nb2[0] = (SLOT + 7, -4)
    bits2[unnamed] ^= 0xFF
    ret2, rec2, pay2, cnt2 = run_fan(host, (bits2, nb2, source, dst_stream, send, seq_base), full_r, full_b)
    assert ret == ret2 == 0 and np.array_equal(rec, rec2) and np.array_equal(pay, pay2) and np.array_equal(cnt, cnt2)


def test_fanout_refusals(host, fan_case):
    bits, nbytes, source, dst_stream, send, seq_base = fan_case
    rec = np.full((50, 5), R_FILL, np.int32)
    pay = np.full(500, P_FILL, np.uint8)
    cnt = np.full(8, FILL_C, np.int32)

    def call(bits=ptr(bits), nbytes=ptr(nbytes), n_src=10, source=ptr(source), n_dst=20, P=5, records=ptr(rec), max_records=50, payload=ptr(pay), cap=500,
             count=ptr(cnt)):
        return host.emu_send_fanout(bits, nbytes, n_src, source, ptr(dst_stream), n_dst, ptr(send), P, SLOT, HBB, ptr(seq_base), 0, records, max_records,
                                    payload, cap, count)

    assert call(bits=None) == -1 and call(nbytes=None) == -1 and call(source=None) == -1 and call(records=None) == -1 and call(payload=None) == -1
    assert call(count=None) == -1
    assert call(n_src=0) == -1 and call(n_src=-1) == -1 and call(n_dst=0) == -1 and call(n_dst=-5) == -1 and call(P=0) == -1 and call(P=-1) == -1
    assert call(max_records=-1) == -1 and call(cap=-1) == -1
    assert call(n_dst=2 ** 15, P=2 ** 15) == -1                                          # n_dst x n_packets x 2 = 2^31
    assert (rec == R_FILL).all() and (pay == P_FILL).all() and (cnt == FILL_C).all()
    # a source row outside [-1, n_src): found by the first pass, records = -1 and nothing else
    for bad in (10, -2, 2 ** 31 - 1, -2 ** 31):
        src = source.copy()
        src[7] = bad
        assert call(source=ptr(src)) == -2
        assert cnt[0] == -1 and (cnt[1:] == FILL_C).all() and (rec == R_FILL).all() and (pay == P_FILL).all()
        assert model_fanout(bits, nbytes, src, HBB)["count"]["records"] == -1
        cnt[0] = FILL_C
    assert call() == 0 and 0 < cnt[0] <= 50

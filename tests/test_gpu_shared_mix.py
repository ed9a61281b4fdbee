"""Shared listener mixes on the GPU (solo_mix_shared, solo_send_fanout through the binding and the raw C ABI): everything against the
independent model of tests/shared_mix_model.py on the small families, against solo_mix itself (every row hears through `source` what
solo_mix gives it), one room of 2048 (the parallel energy pass), the refusals, and the whole shared tick -- decode -> mix_shared -> two
encodes -> fan-out -> ring -> play-out -- against the compiled reference codec around the model.  All comparisons are exact."""
import numpy as np
import pytest

import refcodec as R
from shared_mix_model import fanout_case, heard, model_fanout, model_mix_shared, shared_case

need_ref = pytest.mark.skipif(not R.have_ref("fix"), reason="oracle/_ref not present")
pytestmark = pytest.mark.gpu
FILL = dict(pcm_spk=0x1234, spk_list=-7001, spk_rows=-7002, pcm_room=0x4321, room_list=-7003, source=-7004, energy=-77, mixed=0xA5)
FILL_C = 0x5A5A5A5A
GUARD = 2
FRONT_END_BYTES = 252            # what the receiver front end takes per packet (tests/test_gpu_rate_range.py pins it)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch


def _handle(L, n=4, **kw):
    import solo_amd
    samplerate, framesize_ms = {640: (16000, 40), 1280: (32000, 40), 320: (16000, 20)}[L]
    kw.setdefault("encoder", False)
    h = solo_amd.SoloBatch(n, samplerate=samplerate, framesize_ms=framesize_ms, **kw)
    assert h.packet_samples == L
    return h


def _buffers(torch, n, n_rooms, P, L, guard=GUARD):
    """the outputs of a raw call, pre-filled, with guard rows behind each"""
    dt = dict(pcm_spk=torch.int16, spk_list=torch.int32, spk_rows=torch.int32, pcm_room=torch.int16, room_list=torch.int32, source=torch.int32,
              energy=torch.int64, mixed=torch.uint8)
    shapes = dict(pcm_spk=(n + guard, P, L), spk_list=(n + guard,), spk_rows=(n + guard,), pcm_room=(n_rooms + guard, P, L),
                  room_list=(n_rooms + guard,), source=(n + guard,), energy=(n + guard, P), mixed=(n + guard, P))
    b = {k: torch.full(s, FILL[k], dtype=dt[k], device="cuda") for k, s in shapes.items()}
    b["count"] = torch.full((6,), FILL_C, dtype=torch.int32, device="cuda")
    return b


def _raw(h, d_pcm, d_room, n_rooms, d_gain, K, d_keep, d_slots, b, n=None, P=None):
    ptr = lambda x: None if x is None else x.data_ptr()
    n = d_pcm.shape[0] if n is None else n
    P = d_pcm.shape[1] if P is None else P
    return h.lib.solo_mix_shared(h.h, d_pcm.data_ptr(), n, P, d_room.data_ptr(), n_rooms, ptr(d_gain), K, ptr(d_keep), ptr(d_slots),
                                 b["pcm_spk"].data_ptr(), b["spk_list"].data_ptr(), b["spk_rows"].data_ptr(), b["pcm_room"].data_ptr(),
                                 b["room_list"].data_ptr(), b["source"].data_ptr(), b["energy"].data_ptr(), b["mixed"].data_ptr(),
                                 b["count"].data_ptr(), h._stream())


def _untouched(b, count_from=1):
    return all(bool((b[k] == FILL[k]).all()) for k in FILL) and bool((b["count"][count_from:] == FILL_C).all())


def _compare_raw(torch, h, pcm, room, n_rooms, gain, K, keep, slots):
    """a raw call into pre-filled buffers with guard rows; every array, the fill behind the counts included, against the model"""
    n, P, L = pcm.shape
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    b = _buffers(torch, n, n_rooms, P, L)
    assert _raw(h, up(pcm), up(room), n_rooms, up(gain), K, up(keep), up(slots), b) == 0
    c = h.mix_shared_count(b["count"])
    fill = {k: np.full(tuple(v.shape), FILL[k], v.cpu().numpy().dtype) for k, v in b.items() if k != "count"}
    pad = lambda a, m, v=0: None if a is None else np.concatenate([a, np.full((m - len(a),) + a.shape[1:], v, a.dtype)])
    # (the model sees the guard rows as rows in no room and as rooms without members: nothing of theirs may be written)
    want = model_mix_shared(pad(pcm, n + GUARD), pad(room, n + GUARD, -1), n_rooms + GUARD, pad(gain, n + GUARD), K, pad(keep, n + GUARD),
                            None if slots is None else np.concatenate([slots, slots[-1] + 1 + np.arange(GUARD, dtype=slots.dtype)]), fill=fill)
    want["source"][want["source"] >= n + GUARD] -= GUARD              # (the call has n rows: the room rows of its table start at n ...
    want["source"][n:] = FILL["source"]                              #  ... and the guards are not even marked -1)
    print("solo_mix_shared %d x %d x %d, max_speakers %d: count %s" % (n, P, L, K, c))
    assert c == want["count"], (c, want["count"])
    for k in FILL:
        bad = np.argwhere(b[k].cpu().numpy() != want[k])
        assert len(bad) == 0, (k, bad[:6].tolist())
    return want


@pytest.mark.parametrize("L,P,K", [(320, 3, 3), (640, 1, 3), (640, 3, 3), (1280, 3, 3), (1280, 1, 3), (640, 3, 1), (640, 3, 2)])
def test_gpu_mix_shared_against_model_and_solo_mix(torch_cuda, L, P, K):
    """(a) the small family with everything the interface names, n <= 256; (b) every row hears through `source` what solo_mix gives it"""
    torch = torch_cuda
    pcm, room, gain, n_rooms, keep, slots, marks = shared_case(400 + L + P + K, P, L, K)
    n = len(room)
    assert n <= 256
    h = _handle(L)
    want = _compare_raw(torch, h, pcm, room, n_rooms, gain, K, keep, slots)
    c = want["count"]
    assert c["clipped"] > 0 and 0 < c["shared"] < c["rooms"] and 0 < c["speakers"] < c["rows"]
    _compare_raw(torch, h, pcm, room, n_rooms, None, K, None, None)
    # through the binding, against solo_mix with the same arguments
    d_pcm, d_room, d_gain = torch.from_numpy(pcm).cuda(), torch.from_numpy(room).cuda(), torch.from_numpy(gain).cuda()
    out, mcnt = h.mix(d_pcm, d_room, gain=d_gain, max_speakers=K)
    pcm_spk, spk_list, spk_rows, pcm_room, room_list, source, cnt = h.mix_shared(d_pcm, d_room, gain=d_gain, max_speakers=K,
                                                                                 keep=torch.from_numpy(keep).cuda(), slots=torch.from_numpy(slots).cuda())
    got = dict(pcm_spk=pcm_spk.cpu().numpy(), pcm_room=pcm_room.cpu().numpy(), source=source.cpu().numpy())
    assert h.mix_shared_count(cnt) == c and tuple(pcm_room.shape) == (n, P, L)
    ho = out.cpu().numpy()
    assert np.array_equal(heard(got, n)[room >= 0], ho[room >= 0])
    assert np.array_equal(spk_list.cpu().numpy()[:c["speakers"]], slots[spk_rows.cpu().numpy()[:c["speakers"]]])
    h.close()


def test_gpu_one_large_room(torch_cuda):
    """(c) 2048 rows in ONE room, three speakers: the energy pass runs a wavefront per row, the write-out touches four rows"""
    torch = torch_cuda
    rng = np.random.default_rng(77)
    n, P, L, K = 2048, 1, 640, 3
    level = rng.integers(0, 10, (n, P, 1))
    pcm = (rng.integers(-32768, 32768, (n, P, L), dtype=np.int16) >> level).astype(np.int16)
    pcm[7] = rng.integers(-32768, 32768, (P, L), dtype=np.int16) | 0x2000
    pcm[[100, 1900, 2000]] = pcm[7]                                   # four identical rows, the loudest: the row index decides who is left out
    gain = rng.integers(-100, 8192, n).astype(np.int16)
    gain[[7, 100, 1900, 2000]] = 32767
    room = np.zeros(n, np.int32)
    keep = np.zeros(n, np.uint8)
    keep[[5, 2047]] = 1
    h = _handle(L)
    want = _compare_raw(torch, h, pcm, room, 1, gain, K, keep, None)
    assert want["count"] == dict(rows=n, rooms=1, speakers=5, shared=1, clipped=want["count"]["clipped"])
    assert want["spk_rows"][:5].tolist() == [5, 7, 100, 1900, 2047] and want["mixed"][[7, 100, 1900]].all() and not want["mixed"][2000].any()
    h.close()


def test_gpu_mix_shared_refusals(torch_cuda):
    """(d) the host refuses with -1 and enqueues nothing; a device refusal writes rows = -1 and nothing else"""
    torch = torch_cuda
    P, L, K = 2, 640, 3
    pcm, room, gain, n_rooms, keep, slots, _ = shared_case(14, P, L, K, big=12)
    n = len(room)
    h = _handle(L)
    d_pcm, d_room, d_slots = torch.from_numpy(pcm).cuda(), torch.from_numpy(room).cuda(), torch.from_numpy(slots).cuda()
    b = _buffers(torch, n, n_rooms, P, L)
    call = lambda K=K, n_rooms=n_rooms, bufs=b, pin=d_pcm, **kw: _raw(h, pin, d_room, n_rooms, None, K, None, d_slots, bufs, **kw)
    assert call(K=0) == -1 and call(K=65) == -1 and call(n_rooms=0) == -1 and call(n_rooms=n + 1) == -1 and call(n=0) == -1 and call(P=0) == -1
    assert call(n=2, P=2 ** 30, n_rooms=1) == -1
    assert call(bufs=dict(b, pcm_spk=b["pcm_spk"][0, 0, 4:])) == -1                               # not 16-byte aligned
    assert call(bufs=dict(b, pcm_room=d_pcm)) == -1 and call(bufs=dict(b, pcm_spk=d_pcm[n - 1:])) == -1          # overlap with the input
    assert call(bufs=dict(b, pcm_room=b["pcm_spk"][n - 1:])) == -1                                # ... and of the outputs
    import ctypes as C
    null = C.c_void_p(None)

    class _Null:
        def data_ptr(self):
            return null

    for k in ("pcm_spk", "spk_list", "pcm_room", "room_list", "source", "count"):
        assert call(bufs=dict(b, **{k: _Null()})) == -1, k
    torch.cuda.synchronize()
    assert _untouched(b, 0)
    for what in ("room_low", "room_high", "slots_negative", "slots_equal"):
        r2, s2 = room.copy(), slots.copy()
        if what == "room_low":
            r2[3] = -2
        elif what == "room_high":
            r2[n - 1] = n_rooms
        elif what == "slots_negative":
            s2[0] = -1
        else:
            s2[n - 1] = s2[n - 2]
        assert _raw(h, d_pcm, torch.from_numpy(r2).cuda(), n_rooms, None, K, None, torch.from_numpy(s2).cuda(), b) == 0
        torch.cuda.synchronize()
        assert int(b["count"][0]) == -1 and _untouched(b), what
        assert h.mix_shared_count(b["count"])["rows"] == -1
        b["count"][0] = FILL_C
    # the handle mixes on afterwards
    assert call() == 0
    assert h.mix_shared_count(b["count"])["rows"] == int((room >= 0).sum())
    h.close()


@pytest.mark.parametrize("n_src,n_dst,P", [(10, 20, 5), (120, 300, 5)])
def test_gpu_fanout_against_model(torch_cuda, n_src, n_dst, P):
    """the fan-out family (one tile of packets, and several): DTX and invalid records in named rows, garbage in rows nobody names, masks
    0 .. 3, shared sources, source -1, both caps cutting inside a tick, caps of 0; then a source outside [-1, n_src)"""
    torch = torch_cuda
    h = _handle(640)
    S, hbb = h.slot, 8
    case = fanout_case(31, n_src, n_dst, P, S, hbb)
    bits, nbytes, source, dst_stream, send, seq_base = case
    d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in case]
    full = model_fanout(bits, nbytes, source, hbb, dst_stream=dst_stream, send=send, seq_base=seq_base, first_seq=500)
    need_r, need_b = full["count"]["records_needed"], full["count"]["bytes_needed"]
    assert full["count"]["empty"] >= 5 and full["count"]["refused"] >= 4 and len(set(full["all_records"][:, 3].tolist())) < need_r
    for max_records, cap in [(2 * n_dst * P, n_src * P * S), (need_r, need_b), (need_r // 3 + 1, need_b), (need_r, need_b * 2 // 5 + 1),
                             (need_r // 3, need_b // 2), (0, need_b), (need_r, 0), (0, 0)]:
        rec = torch.full((max_records + GUARD, 5), -9, dtype=torch.int32, device="cuda")
        pay = torch.full((cap + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
        want = model_fanout(bits, nbytes, source, hbb, dst_stream=dst_stream, send=send, seq_base=seq_base, first_seq=500, max_records=max_records,
                            cap=cap, records=np.full((max_records + GUARD, 5), -9, np.int32), payload=np.full(cap + GUARD, 0xEE, np.uint8))
        r, p, cnt = h.send_fanout(d[0], d[1], d[2], dst_stream=d[3], send=d[4], first_seq=500, seq_base=d[5], records=rec[:max_records], payload=pay[:cap])
        c = h.send_count(cnt)
        print("solo_send_fanout caps (%d, %d): %s" % (max_records, cap, c))
        assert c == want["count"], (max_records, cap, c, want["count"])
        assert np.array_equal(rec.cpu().numpy(), want["records"]) and np.array_equal(pay.cpu().numpy(), want["payload"]), (max_records, cap)
    # the defaults: no stream numbers, masks or sequence bases, buffers of the binding
    want = model_fanout(bits, nbytes, source, hbb)
    r, p, cnt = h.send_fanout(d[0], d[1], d[2])
    assert h.send_count(cnt) == want["count"] and np.array_equal(r.cpu().numpy(), want["records"]) and np.array_equal(p.cpu().numpy(), want["payload"])
    # refused on the device: records = -1, nothing else
    rec = torch.full((50, 5), -9, dtype=torch.int32, device="cuda")
    pay = torch.full((4000,), 0xEE, dtype=torch.uint8, device="cuda")
    for bad in (n_src, -2, 2 ** 31 - 1):
        src = source.copy()
        src[11] = bad
        r, p, cnt = h.send_fanout(d[0], d[1], torch.from_numpy(src).cuda(), records=rec, payload=pay)
        hc = cnt.cpu().numpy()
        assert hc[0] == -1 and (hc[1:] == 0).all() and bool((rec == -9).all()) and bool((pay == 0xEE).all()), bad
    lib, z = h.lib, d[0].data_ptr()
    assert lib.solo_send_fanout(h.h, z, d[1].data_ptr(), 0, d[2].data_ptr(), None, n_dst, None, P, None, 0, rec.data_ptr(), 50, pay.data_ptr(), 4000, cnt.data_ptr(), None) == -1
    assert lib.solo_send_fanout(h.h, z, d[1].data_ptr(), n_src, None, None, n_dst, None, P, None, 0, rec.data_ptr(), 50, pay.data_ptr(), 4000, cnt.data_ptr(), None) == -1
    assert lib.solo_send_fanout(h.h, z, d[1].data_ptr(), n_src, d[2].data_ptr(), None, 2 ** 15, None, 2 ** 15, None, 0, rec.data_ptr(), 50, pay.data_ptr(), 4000, cnt.data_ptr(), None) == -1
    h.close()


@need_ref
def test_gpu_shared_tick_against_the_compiled_reference(torch_cuda):
    """(e) 24 participants in rooms of 1, 2, 5, 8 and 8, two speakers per room, six one-packet ticks with the talkers changing and a
    one-tick hangover as d_keep: decode -> mix_shared -> encode the speakers on the participants' handle and the rooms on a rooms handle
    into one table -> send_fanout -> the ring of a receiving handle -> play-out.  The payload of every speaker slot and every room slot
    must be what a reference encoder gives that is fed the model's PCM in the ticks in which the slot was listed, and every participant
    must play what a reference decoder makes of the payloads the model says it was sent."""
    import solo_amd
    torch = torch_cuda
    N, T_, K, FIRST, L = 24, 6, 2, 900, 640
    n_rooms = 5
    room = np.repeat(np.arange(n_rooms), (1, 2, 5, 8, 8)).astype(np.int32)[np.random.default_rng(4).permutation(N)]
    rng = np.random.default_rng(23)
    talk = rng.random((N, T_)) < 0.35
    talk[:, 0] |= rng.random(N) < 0.3
    x = np.stack([R.synth_stream(800 + i, T_) for i in range(N)])
    x = np.where(talk[:, :, None], x, x >> 9).astype(np.int16)          # those who do not talk murmur
    # what the participants sent: the reference encoder per participant
    S = solo_amd.DEFAULT_SLOT_BYTES
    in_bits, in_nb = np.zeros((N, T_, S), np.uint8), np.zeros((N, T_, 2), np.int16)
    ref_heard = np.zeros((N, T_, L), np.int16)
    for i in range(N):
        e, d = R.RefEncoder("fix"), R.RefDecoder("fix")
        for t in range(T_):
            pl, n0, n1 = e.encode(x[i, t])
            in_bits[i, t, :n0] = np.frombuffer(pl, np.uint8)
            in_nb[i, t] = (n0, n1)
            ref_heard[i, t], ret = d.decode(pl, n0, n1, 4)
            assert ret == 0
    bridge = solo_amd.SoloBatch(N, encoder=True, decoder=True)         # the participants' handle
    rooms = solo_amd.SoloBatch(n_rooms, encoder=True, decoder=False)    # one slot per room
    rx = solo_amd.SoloBatch(N, encoder=False, decoder=True)            # the far ends
    rx.recv_create(4, 256, 0)
    rx.recv_reset_streams(list(range(N)), FIRST)
    d_room = torch.from_numpy(room).cuda()
    enc_spk = [R.RefEncoder("fix") for _ in range(N)]
    enc_room = [R.RefEncoder("fix") for _ in range(n_rooms)]
    dec = [R.RefDecoder("fix") for _ in range(N)]
    keep = np.zeros(N, np.uint8)
    sources_seen, switched = set(), 0
    last_source = None
    for t in range(T_):
        pcm, st = bridge.decode(torch.from_numpy(in_bits[:, t:t + 1].copy()).cuda(), torch.from_numpy(in_nb[:, t:t + 1].copy()).cuda())
        pcm_spk, spk_list, spk_rows, pcm_room, room_list, source, cnt = bridge.mix_shared(pcm, d_room, max_speakers=K, keep=torch.from_numpy(keep).cuda(),
                                                                                         n_rooms=n_rooms)
        c = bridge.mix_shared_count(cnt)                              # the 24-byte read-back of the tick
        assert int(st.abs().max()) == 0 and np.array_equal(pcm.cpu().numpy()[:, 0], ref_heard[:, t])
        want = model_mix_shared(ref_heard[:, t:t + 1], room, n_rooms, None, K, keep)
        ns, nr = want["count"]["speakers"], want["count"]["shared"]
        assert c == want["count"] and 0 < ns < N and 0 < nr <= n_rooms
        assert np.array_equal(spk_list.cpu().numpy()[:ns], want["spk_list"][:ns]) and np.array_equal(room_list.cpu().numpy()[:nr], want["room_list"][:nr])
        assert np.array_equal(source.cpu().numpy(), want["source"])
        assert np.array_equal(pcm_spk.cpu().numpy()[:ns], want["pcm_spk"][:ns]) and np.array_equal(pcm_room.cpu().numpy()[:nr], want["pcm_room"][:nr])
        # one table: the speakers' packets in rows 0 .., the rooms' in rows N ..; rows nobody names keep 0xA5 length words
        bits = torch.zeros((N + n_rooms, 1, S), dtype=torch.uint8, device="cuda")
        nb = torch.full((N + n_rooms, 1, 2), -23131, dtype=torch.int16, device="cuda")
        _, _, st1 = bridge.encode(pcm_spk[:ns], bits=bits[:ns], nbytes=nb[:ns], streams=spk_list[:ns])
        _, _, st2 = rooms.encode(pcm_room[:nr], bits=bits[N:N + nr], nbytes=nb[N:N + nr], streams=room_list[:nr])
        rec, pay, scnt = bridge.send_fanout(bits, nb, source, first_seq=FIRST + t)
        sc = bridge.send_count(scnt)
        assert int(st1.abs().max()) == 0 and int(st2.abs().max()) == 0 and sc["refused"] == 0 and sc["empty"] == 0
        assert sc["records"] == sc["records_needed"] > N and sc["bytes"] == sc["bytes_needed"]
        hb, hn = bits.cpu().numpy(), nb.cpu().numpy()
        assert int(hn[:ns, 0, 0].max()) <= FRONT_END_BYTES
        # every slot that was listed against its reference encoder
        table = {}
        for k in range(ns):
            pl, n0, n1 = enc_spk[int(want["spk_list"][k])].encode(want["pcm_spk"][k, 0])
            table[k] = (pl, n0, n1)
        for j in range(nr):
            pl, n0, n1 = enc_room[int(want["room_list"][j])].encode(want["pcm_room"][j, 0])
            table[N + j] = (pl, n0, n1)
        for row, (pl, n0, n1) in table.items():
            assert (int(hn[row, 0, 0]), int(hn[row, 0, 1])) == (n0, n1) and hb[row, 0, :n0].tobytes() == pl, (t, row)
        # the records and the pool against the model: every source packet is in the pool once, shared by the records of its listeners
        fan = model_fanout(hb, hn, want["source"], 8, first_seq=FIRST + t)
        hr = rec.cpu().numpy()
        assert sc == fan["count"] and np.array_equal(hr, fan["records"]) and np.array_equal(pay.cpu().numpy(), fan["payload"])
        assert sc["bytes"] <= sum(n0 for _, n0, _ in table.values()) and len(set(hr[:sc["records"], 3].tolist())) < sc["records"]
        # the far ends: all records of the tick into the ring, one packet played
        before = rx.recv_stats()
        rx.recv_insert(rec[:sc["records"]].contiguous(), pay)
        after = rx.recv_stats()
        assert after["inserted"] - before["inserted"] == sc["records"] and after["bad"] == after["late"] == after["ahead"] == after["duplicate"] == 0
        played, st3 = rx.recv_decode(1)
        hp = played.cpu().numpy()
        assert int(st3.abs().max()) == 0
        for i in range(N):
            pl, n0, n1 = table[int(want["source"][i])]
            ref_pcm, ret = dec[i].decode(pl, n0, n1, 4)
            assert ret == 0 and np.array_equal(hp[i, 0], ref_pcm), (t, i)
        src_now = want["source"].copy()
        sources_seen |= {"speaker" if s < N else "room" for s in src_now.tolist()}
        if last_source is not None:
            switched += int(((last_source < N) != (src_now < N)).sum())
        last_source = src_now
        keep = want["mixed"][:, 0].copy()                              # the hangover: who was picked in this tick keeps its encoder in the next
    assert sources_seen == {"speaker", "room"} and switched > 0         # listeners moved between a shared encoder and their own
    for h in (bridge, rooms, rx):
        h.close()

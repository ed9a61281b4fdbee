"""RTP framing and parsing on the GPU (solo_rtp_pack / solo_rtp_parse through solo_amd.Rtp and the C ABI) against the independent model of
tests/rtp_model.py: synthetic records at the tile boundaries of the pack passes (1, 257 = one 256-record tile and a record, 16 385 = 65
tiles, so the scanning wavefront takes a second round of 64), with and without levels and with both caps cutting inside the output; the
records of a real solo_send_fanout; hostile datagrams shuffled among valid ones; the end-to-end chain encode -> send_pack -> rtp_pack ->
shuffle and loss -> rtp_parse -> recv_insert -> recv_decode against the raw-record path and against solo_batch_decode; the binding
errors; and both halves captured in a graph and replayed against eager twins.

CAPTURED names the test that captures each of the two calls the interface calls capturable (tests/test_rtp_model.py holds this file to it)."""
import numpy as np
import pytest

import graph_replay_lib as G
import rtp_model as M
import solo_testlib as T

pytestmark = pytest.mark.gpu
CAPTURED = {"solo_rtp_pack": "test_capture_send_pack_and_rtp_pack", "solo_rtp_parse": "test_capture_rtp_parse_and_recv_insert"}
FILL_D, FILL_W = -7, 0xA5
FRONT_END_BYTES = 252            # what the receiver front end takes per packet (tests/test_gpu_rate_range.py pins it)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(torch, t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def gpu_session(ses):
    """a solo_amd.Rtp bound as the model's session dict says"""
    import solo_amd
    r = solo_amd.Rtp(ses["n_streams"], ses["L"])
    s = sorted(ses["streams"])
    if s:
        c = [ses["streams"][k] for k in s]
        r.bind(s, [x["ssrc"] for x in c], [x["ts_offset"] for x in c], [x["seq_offset"] for x in c], [x["pt"] for x in c], ses["level_id"])
    return r


def ring_handle(N, play, samplerate=16000, md=None, depth=8):
    """a decoder handle with a ring whose play-out positions are `play`"""
    import solo_amd
    h = solo_amd.SoloBatch(N, encoder=False, decoder=True, samplerate=samplerate)
    if md is not None:
        h.reset_streams(list(range(N)), use_md_index=[int(v) for v in md], which="dec")
    h.recv_create(depth, 256, 0)
    h.recv_reset_streams(list(range(N)), [int(v) for v in play])
    return h


def pack_and_compare(torch, rtp, ses, rec, n_rec, pool, level, max_records=None, cap=None):
    """rtp.pack into guarded buffers; d_dgrams, d_wire, the count and the guards against the model -> (dgrams, wire, count, model)"""
    m = rec.shape[0] if max_records is None else max_records
    cp = 4 * (int(pool.size) + 23 * m) if cap is None else cap
    GUARD = 64
    send_count = np.zeros(8, np.int32)
    send_count[0] = n_rec
    dg = torch.full((m + GUARD, 2), FILL_D, dtype=torch.int32, device="cuda")
    wire = torch.full((cp + GUARD,), FILL_W, dtype=torch.uint8, device="cuda")
    d, w, cnt = rtp.pack(dev(torch, rec[:m]), dev(torch, send_count), dev(torch, pool), level=None if level is None else dev(torch, level),
                         dgrams=dg[:m], wire=wire[:cp])
    c = rtp.pack_count(cnt)
    want = M.model_pack(ses, rec, n_rec, pool, level, m, cp)
    print("rtp_pack %d records (max %d, cap %d): %s" % (n_rec, m, cp, c))
    assert c == want["count"], (c, want["count"])
    hd, hw = dg.cpu().numpy(), wire.cpu().numpy()
    n = min(n_rec, m)
    assert np.array_equal(hd[:n], want["dgrams"])
    assert np.array_equal(hw[:c["bytes"]], want["wire"])
    assert (hd[n:] == FILL_D).all() and (hw[c["bytes"]:] == FILL_W).all()      # nothing behind what was written, nor behind the caps
    return hd[:n], hw[:cp], c, want


# ---- synthetic pack ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 257, 16385])
def test_synthetic_pack(torch_cuda, n):
    torch = torch_cuda
    rng = np.random.default_rng(700 + n)
    ses = M.random_session(rng, 12, 640, 9, unbound=(3, 8), equal_pt=(5,))
    rtp = gpu_session(ses)
    pool_bytes, depth = 50021, 7
    pool = rng.integers(0, 256, pool_bytes, dtype=np.uint8)
    rec = M.random_records(rng, ses, n, pool_bytes, seq_hi=2 ** 31, hostile=n > 1)
    if n == 1:
        rec[0, 0] = 4                                             # (a bound stream)
    level = rng.integers(0, 256, (12, depth), dtype=np.uint8)
    _, _, c, _ = pack_and_compare(torch, rtp, ses, rec, n, pool, None)
    _, _, cl, full = pack_and_compare(torch, rtp, ses, rec, n, pool, level)
    assert cl["dgrams"] == cl["dgrams_needed"] == c["dgrams"] > 0 and cl["bytes"] > c["bytes"]
    if n > 1:
        assert all(full["reasons"].get(r, 0) > 0 for r in ("stream", "unbound", "desc", "seq", "len", "long", "range")), full["reasons"]
        assert cl["refused"] > n // 10
    # both caps cut inside the output: the wire cap inside a header, a byte short of a datagram's end and between its end and its pad
    # bytes; max_records two thirds in; and both at once
    alld = full["all_dgrams"]
    valid = np.nonzero(alld[:, 1] > 0)[0]
    k = int(valid[len(valid) // 2])
    odd = [int(v) for v in valid if alld[v, 1] % 4]
    caps = [(n, int(alld[k, 0] + 5)), (n, int(alld[k, 0] + alld[k, 1] - 1)), (n, 0)]
    if odd:
        caps.append((n, int(alld[odd[len(odd) // 2]].sum())))
    if n > 1:
        caps += [(2 * n // 3, None), (2 * n // 3, int(alld[valid[len(valid) // 3], 0] + 13)), (n - 1, cl["bytes_needed"])]
    for m, cp in caps:
        _, _, cc, _ = pack_and_compare(torch, rtp, ses, rec, n, pool, level, m, cp)
        assert cc["dgrams"] < cl["dgrams"] or (m, cp) == (n - 1, cl["bytes_needed"])
        if m == n:
            assert cc["dgrams_needed"] == cl["dgrams_needed"] and cc["bytes_needed"] == cl["bytes_needed"] and cc["refused"] == cl["refused"]
    # the sender's count says fewer records than the buffer holds; and a refused list
    if n > 1:
        pack_and_compare(torch, rtp, ses, rec, 256, pool, level)
        pack_and_compare(torch, rtp, ses, rec, n + 9, pool, level)
    send_count = dev(torch, np.array([-1, 0, 0, 0, 0, 0, 0, 0], np.int32))
    dg = torch.full((n, 2), FILL_D, dtype=torch.int32, device="cuda")
    wire = torch.full((4096,), FILL_W, dtype=torch.uint8, device="cuda")
    _, _, cnt = rtp.pack(dev(torch, rec), send_count, dev(torch, pool), dgrams=dg, wire=wire)
    assert rtp.pack_count(cnt)["dgrams"] == -1 and host(torch, cnt)[1:].tolist() == [0] * 7
    assert bool((dg == FILL_D).all()) and bool((wire == FILL_W).all())
    # host refusals of the C ABI on a live session
    L, r5, p5 = rtp.lib, dev(torch, rec), dev(torch, pool)
    a = lambda **k: [k.get("rec", r5.data_ptr()), k.get("sc", send_count.data_ptr()), k.get("m", n), p5.data_ptr(), k.get("pb", pool_bytes), k.get("lv", None),
                     k.get("depth", 0), k.get("dg", dg.data_ptr()), k.get("wire", wire.data_ptr()), k.get("cap", 4096), k.get("cnt", cnt.data_ptr()), None]
    lv = dev(torch, level)
    for bad in (dict(rec=None), dict(sc=None), dict(m=0), dict(m=-1), dict(pb=-1), dict(cap=-1), dict(dg=None), dict(wire=None), dict(cnt=None),
                dict(lv=lv.data_ptr(), depth=0), dict(wire=wire.data_ptr() + 1), dict(dg=dg.data_ptr() + 2), dict(cnt=cnt.data_ptr() + 4), dict(rec=r5.data_ptr() + 1)):
        assert L.solo_rtp_pack(rtp.h, *a(**bad)) == -1, bad
    assert L.solo_rtp_pack(None, *a()) == -1
    torch.cuda.synchronize()
    rtp.close()


def test_fanout_shaped_pack(torch_cuda):
    """8 destinations share 2 sources' offsets: the records and the count come from solo_send_fanout on the device, every destination's
    copy gets its own header"""
    import solo_amd
    torch = torch_cuda
    rng = np.random.default_rng(17)
    P, slot = 3, 128
    tx = solo_amd.SoloBatch(8, encoder=False, decoder=True, slot_bytes=slot)
    bits = rng.integers(0, 256, (2, P, slot), dtype=np.uint8)
    nb = np.zeros((2, P, 2), np.int16)
    nb[:, :, 0] = rng.integers(60, 120, (2, P))
    nb[:, :, 1] = nb[:, :, 0] // 2 - rng.integers(0, 9, (2, P))
    source = np.array([0, 1, 0, 1, 0, 1, 0, 1], np.int32)
    records, payload, scount = tx.send_fanout(dev(torch, bits), dev(torch, nb), dev(torch, source), first_seq=40)
    sc = tx.send_count(scount)
    assert sc["records"] == 8 * P * 2 and sc["bytes"] == int(nb[:, :, 0].sum())
    ses = M.random_session(rng, 8, 640, 0)
    rtp = gpu_session(ses)
    wire = torch.full((16384,), FILL_W, dtype=torch.uint8, device="cuda")
    dg, w, cnt = rtp.pack(records, scount, payload, wire=wire)
    c = rtp.pack_count(cnt)
    rec = host(torch, records)
    assert len({(int(a), int(b)) for a, b in rec[:sc["records"], 3:5]}) == 2 * P * 2            # offsets do repeat
    want = M.model_pack(ses, rec, sc["records"], host(torch, payload), None)
    assert c == want["count"] and c["dgrams"] == 48 and c["refused"] == 0 and c["bytes"] > 4 * sc["bytes"]
    assert np.array_equal(host(torch, dg)[:48], want["dgrams"]) and np.array_equal(host(torch, w)[:c["bytes"]], want["wire"])
    assert bool((w[c["bytes"]:] == FILL_W).all())
    rtp.close()
    tx.close()


# ---- synthetic parse ----------------------------------------------------------------------------------------------------------------------------
def _mixed_datagrams(rng, ses, play, n):
    """n datagrams: with n >= 65 every hostile kind at least once, the rest valid ones of the bound streams (with and without a level,
    both descriptions, 0 .. 6 packets ahead of the play-out position); shuffled"""
    bound = sorted(ses["streams"])
    out = []
    if n >= 65:
        while len(out) < n // 3:
            for s in (2, 5):
                out += [k[1] for k in M.hostile_kinds(ses, play, s, rng)]
        out = out[:max(n // 3, 45)]
        assert len(out) >= len(M.hostile_kinds(ses, play, 2, rng))
    while len(out) < n:
        s = int(rng.choice(bound))
        c = ses["streams"][s]
        seq = int(play[s]) + int(rng.integers(0, 7))
        ext = M.level_ext(ses["level_id"], int(rng.integers(0, 256))) if rng.random() < 0.6 else None
        out.append(M.build(c["ssrc"], c["pt"][int(rng.integers(0, 2))], int(rng.integers(0, 65536)), c["ts_offset"] + seq * ses["L"],
                           rng.integers(0, 256, int(rng.integers(1, 100)), dtype=np.uint8).tobytes(), ext=ext))
    order = rng.permutation(n)
    return [out[i] for i in order]


def _lay_out(rng, dgs):
    wire, table = bytearray(b"\x11" * 3), []
    for d in dgs:
        wire += b"\x22" * int(rng.integers(0, 4))                 # (every byte alignment)
        table.append((len(wire), len(d)))
        wire += d
    return np.array(table, np.int32).reshape(-1, 2), np.frombuffer(bytes(wire), np.uint8).copy()


def _check_parse(torch, rtp, batch, ses, play, dg, wire):
    n = dg.shape[0]
    arr = torch.full((n + 8, 5), FILL_D, dtype=torch.int32, device="cuda")
    lv = torch.full((n + 8,), 0x77, dtype=torch.uint8, device="cuda")
    sq = torch.full((n + 8,), 0x7777, dtype=torch.int16, device="cuda")
    a, l, s, cnt = rtp.parse(batch, dev(torch, dg), dev(torch, wire), arrivals=arr[:n], level=lv[:n], rtp_seq=sq[:n])
    c = rtp.parse_count(cnt)
    want = M.model_parse(ses, play, dg, wire)
    print("rtp_parse %d datagrams: %s" % (n, c))
    assert c == want["count"], (c, want["count"])
    ha, hl, hs = arr.cpu().numpy(), lv.cpu().numpy(), sq.cpu().numpy().view(np.uint16)
    assert np.array_equal(ha[:n], want["arrivals"]) and np.array_equal(hl[:n], want["level"]) and np.array_equal(hs[:n], want["rtp_seq"])
    assert (ha[n:] == FILL_D).all() and (hl[n:] == 0x77).all() and (hs[n:] == 0x7777).all()
    return c, want


@pytest.mark.parametrize("n", [1, 65, 4097])
def test_synthetic_parse(torch_cuda, n):
    torch = torch_cuda
    rng = np.random.default_rng(800 + n)
    ses = M.random_session(rng, 6, 640, 5, unbound=(3,), equal_pt=(1,))
    play = rng.integers(0, 5000, 6).astype(np.int32)
    play[4] = 6710886                                             # (seq x 640 crosses 2^32 right here)
    rtp, batch = gpu_session(ses), ring_handle(6, play)
    dg, wire = _lay_out(rng, _mixed_datagrams(rng, ses, play, n))
    c, want = _check_parse(torch, rtp, batch, ses, play, dg, wire)
    if n >= 65:
        assert all(c[v] > 0 for v in M.VERDICTS) and c["with_level"] > 0
        assert (want["arrivals"][:, 2] == -1).any()               # the stream with equal payload types
        # ranges that leave the wire are malformed and never read
        out = np.array([[-1, 40], [wire.size - 39, 40], [wire.size, 12], [2 ** 31 - 1, 2 ** 31 - 1], [0, -5]], np.int32)
        c2, _ = _check_parse(torch, rtp, batch, ses, play, np.concatenate([out, dg[:9]]), wire)
        assert c2["malformed"] >= 5
    # both optional outputs absent: the same arrivals and counts
    a, l, s, cnt = rtp.parse(batch, dev(torch, dg), dev(torch, wire))
    assert l is None and s is None and rtp.parse_count(cnt) == c and np.array_equal(host(torch, a), want["arrivals"])
    # the ring takes the arrivals as they are: the rejected ones are its `bad` (and so are those of the stream with equal payload
    # types, desc = -1, whose decoder runs without useMDIndex here)
    before = batch.recv_stats()
    batch.recv_insert(a, dev(torch, wire))
    after = batch.recv_stats()
    no_index = int((want["arrivals"][:, 2] == -1).sum())
    assert after["bad"] - before["bad"] == n - c["accepted"] + no_index and sum(after.values()) - sum(before.values()) == n
    # host refusals: a handle without a ring, of another size, of another packet length; bad pointers
    import solo_amd
    no_ring = solo_amd.SoloBatch(6, encoder=False, decoder=True)
    other_n = ring_handle(5, play[:5])
    wide = ring_handle(6, play, samplerate=32000)
    L, d5, w5 = rtp.lib, dev(torch, dg), dev(torch, wire)
    args = lambda **k: [k.get("dg", d5.data_ptr()), k.get("n", n), w5.data_ptr(), k.get("wb", wire.size), k.get("arr", a.data_ptr()), None, k.get("sq", None),
                        k.get("cnt", cnt.data_ptr()), None]
    for h in (no_ring, other_n, wide):
        assert L.solo_rtp_parse(rtp.h, h.h, *args()) == -1
    for bad in (dict(dg=None), dict(n=-1), dict(wb=-1), dict(arr=None), dict(cnt=None), dict(dg=d5.data_ptr() + 2), dict(sq=a.data_ptr() + 1)):
        assert L.solo_rtp_parse(rtp.h, batch.h, *args(**bad)) == -1, bad
    assert L.solo_rtp_parse(None, batch.h, *args()) == -1 and L.solo_rtp_parse(rtp.h, None, *args()) == -1
    torch.cuda.synchronize()
    rtp.close()


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------------
def _encoded(torch, N, P, samplerate):
    """N streams x P packets at rates whose packets the receiver front end takes, useMDIndex mixed -> (bits, nbytes on the device, md)"""
    import solo_amd
    from solo_amd.synth import synth_stream
    rates = [9600, 12000, 13600] if samplerate == 16000 else [20000, 24000]
    md = [(k // 3) % 2 for k in range(N)] if N > 2 else [0, 1][:N]
    L = 640 * samplerate // 16000
    enc = solo_amd.SoloBatch(N, rate=rates[-1], encoder=True, decoder=False, samplerate=samplerate)
    enc.reset_streams(list(range(N)), rate=[rates[k % len(rates)] for k in range(N)], dtx=[False] * N, use_md_index=md, which="enc")
    per40 = (samplerate // 16000) * P + 2
    pcm = np.stack([synth_stream(900 + k, per40).reshape(-1)[:P * L].reshape(P, L) for k in range(N)])
    bits, nb, st = enc.encode(dev(torch, pcm))
    torch.cuda.synchronize()
    assert int(st.abs().max()) == 0 and 0 < int(nb[:, :, 0].min()) and int(nb[:, :, 0].max()) <= FRONT_END_BYTES
    enc.close()
    return bits, nb, md


def _decoder(N, samplerate, md):
    import solo_amd
    d = solo_amd.SoloBatch(N, encoder=False, decoder=True, samplerate=samplerate)
    d.reset_streams(list(range(N)), use_md_index=[int(v) for v in md], which="dec")
    return d


@pytest.mark.parametrize("samplerate,N", [(16000, 8), (32000, 2)])
def test_end_to_end(torch_cuda, samplerate, N):
    """encode -> send_pack -> rtp_pack -> shuffle, drop every fifth -> rtp_parse -> recv_insert -> recv_decode: PCM and status bit for bit
    what the same shuffle and drop of the raw records gives through solo_recv_insert, and what solo_batch_decode gives with the
    equivalent mask on a fresh decoder"""
    import solo_amd
    torch = torch_cuda
    rng = np.random.default_rng(samplerate + N)
    P, L, FIRST = 4, 640 * samplerate // 16000, 1000
    bits, nb, md = _encoded(torch, N, P, samplerate)
    eq = md.index(1)                                              # this stream: equal payload types, the description comes from the payload
    base = rng.integers(0, 100000, N).astype(np.int32)
    first = FIRST + base.astype(np.int64)
    ses = M.random_session(rng, N, L, 1, equal_pt=(eq,))
    for s, c in ses["streams"].items():                           # timestamp and 16-bit sequence number both wrap inside the run, at packet 1 / 2
        c["ts_offset"] = int((100 - (int(first[s]) + 2) * L) % 2 ** 32)
        c["seq_offset"] = int((1 - 2 * (int(first[s]) + 2)) % 65536)
    rtp = gpu_session(ses)
    tx = solo_amd.SoloBatch(N, encoder=True, decoder=False, samplerate=samplerate, rate=24000)
    records, payload, scount = tx.send_pack(bits, nb, first_seq=FIRST, seq_base=dev(torch, base))
    sc = tx.send_count(scount)
    n = sc["records"]
    assert n == sc["records_needed"] == 2 * N * P and sc["refused"] == 0
    level = rng.integers(0, 255, (N, P), dtype=np.uint8)          # (255, "voice at -127 dBov", reads back as "no level": not sent here)
    dgrams, wire, cnt = rtp.pack(records, scount, payload, level=dev(torch, level))
    c = rtp.pack_count(cnt)
    rec, dg, hw = host(torch, records)[:n], host(torch, dgrams)[:n], host(torch, wire)
    want = M.model_pack(ses, rec, n, host(torch, payload), level)
    assert c == want["count"] and c["dgrams"] == n and c["refused"] == 0
    assert np.array_equal(dg, want["dgrams"]) and np.array_equal(hw[:c["bytes"]], want["wire"])
    # the network: another order, every fifth datagram lost
    perm = rng.permutation(n)
    keep = np.array([perm[i] for i in range(n) if i % 5 != 4])
    rx = ring_handle(N, first, samplerate, md, depth=P)
    arr, lv, sq, pcnt = rtp.parse(rx, dev(torch, dg[keep]), wire, level=True, rtp_seq=True)
    pc = rtp.parse_count(pcnt)
    assert pc == dict(accepted=len(keep), with_level=len(keep), malformed=0, version=0, unknown_ssrc=0, unknown_pt=0, timestamp=0, reserved=0), pc
    ha, hl, hs = host(torch, arr), host(torch, lv), host(torch, sq).view(np.uint16)
    k = rec[keep]
    assert np.array_equal(ha[:, [0, 1, 4]], k[:, [0, 1, 4]]) and np.array_equal(ha[:, 2], np.where(k[:, 0] == eq, -1, k[:, 2]))
    assert np.array_equal(ha[:, 3], dg[keep, 0] + 20) and (ha[:, 2] == -1).any()
    assert np.array_equal(hl, level[k[:, 0], k[:, 1] % P])
    so = np.array([ses["streams"][int(s)]["seq_offset"] for s in k[:, 0]], np.int64)
    assert np.array_equal(hs, ((so + 2 * k[:, 1].astype(np.int64) + k[:, 2]) % 65536).astype(np.uint16))
    ts = np.array([int.from_bytes(bytes(hw[o + 4:o + 8]), "big") for o in dg[:, 0]], np.int64)
    raw_seq = np.array([int.from_bytes(bytes(hw[o + 2:o + 4]), "big") for o in dg[:, 0]], np.int64)
    for s in range(N):                                            # both did wrap inside the run
        mine = rec[:, 0] == s
        assert ts[mine].max() > 2 ** 32 - 2 * L and ts[mine].min() < 2 * L and raw_seq[mine].max() == 65535 and raw_seq[mine].min() == 0, s
    rx.recv_insert(arr, wire)
    assert rx.recv_stats() == dict(inserted=len(keep), late=0, ahead=0, duplicate=0, bad=0)
    got, st = rx.recv_decode(P)
    got, st = host(torch, got), host(torch, st)
    # 1: the raw records, the same shuffle and drop
    raw = ring_handle(N, first, samplerate, md, depth=P)
    raw.recv_insert(dev(torch, k), payload)
    assert raw.recv_stats() == dict(inserted=len(keep), late=0, ahead=0, duplicate=0, bad=0)
    want1, st1 = raw.recv_decode(P)
    assert np.array_equal(got, host(torch, want1)) and np.array_equal(st, host(torch, st1))
    # 2: solo_batch_decode with the equivalent mask on a fresh decoder
    recv = np.zeros((N, P), np.uint8)
    for s, seq, d in k[:, :3]:
        recv[s, seq - first[s]] |= 1 << d
    assert (recv == 3).any() and (recv != 3).any()                # whole packets, and packets that lost a description (or both)
    want2, st2 = _decoder(N, samplerate, md).decode(bits, nb, dev(torch, recv))
    assert np.array_equal(got, host(torch, want2)) and np.array_equal(st, host(torch, st2))
    assert int(np.abs(st).max()) == 0 and got.any()
    rtp.close()


# ---- binding errors -------------------------------------------------------------------------------------------------------------------------------
def test_binding_errors(torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(5)
    ses = M.random_session(rng, 4, 640, 2)
    play = np.array([10, 20, 30, 40], np.int32)
    rtp, batch = gpu_session(ses), ring_handle(4, play)
    pool = rng.integers(0, 256, 400, dtype=np.uint8)
    rec = np.array([[s, int(play[s]) + p, d, 10 * (4 * s + 2 * p + d), 9 + d] for p in range(2) for s in range(4) for d in (0, 1)], np.int32)
    level = rng.integers(0, 255, (4, 3), dtype=np.uint8)

    def both(ses_now, wire_of=None):
        dg, hw, c, _ = pack_and_compare(torch, rtp, ses_now, rec, 16, pool, level)
        d2, w2 = (dg, hw) if wire_of is None else wire_of
        live = d2[:, 1] > 0
        pc, _ = _check_parse(torch, rtp, batch, ses_now, play, d2[live], w2)
        return dg, hw, c, pc

    dg0, w0, c0, p0 = both(ses)
    assert c0["dgrams"] == 16 and p0["accepted"] == 16 and p0["with_level"] == 16
    # a duplicate SSRC across streams, a bad payload type, a bad level id through the C ABI: refused, and nothing has changed
    with pytest.raises(RuntimeError):
        rtp.bind([1], ses["streams"][2]["ssrc"], level_id=2)
    with pytest.raises(RuntimeError):
        rtp.bind([0, 1], [77, 77], level_id=2)
    import ctypes as C
    one = lambda t, v: (t * 1)(v)
    assert rtp.lib.solo_rtp_bind(rtp.h, one(C.c_int32, 1), 1, one(C.c_uint32, 99), one(C.c_uint32, 0), one(C.c_uint16, 0), one(C.c_uint8, 128), one(C.c_uint8, 97), 2,
                                 None) == -1
    assert rtp.lib.solo_rtp_bind(rtp.h, one(C.c_int32, 1), 1, one(C.c_uint32, 99), one(C.c_uint32, 0), one(C.c_uint16, 0), one(C.c_uint8, 96), one(C.c_uint8, 97), 15,
                                 None) == -1
    assert rtp.lib.solo_rtp_bind(rtp.h, one(C.c_int32, 4), 1, one(C.c_uint32, 99), one(C.c_uint32, 0), one(C.c_uint16, 0), one(C.c_uint8, 96), one(C.c_uint8, 97), 2,
                                 None) == -1
    assert rtp.lib.solo_rtp_unbind(rtp.h, one(C.c_int32, 4), 1, None) == -1 and rtp.lib.solo_rtp_unbind(rtp.h, one(C.c_int32, 1), 0, None) == -1
    dg1, w1, c1, p1 = both(ses)
    assert np.array_equal(dg1, dg0) and np.array_equal(w1, w0) and c1 == c0 and p1 == p0
    # unbind: the stream's records are refused, its datagrams (of the wire packed before) are unknown_ssrc
    rtp.unbind([2])
    less = dict(ses, streams={s: c for s, c in ses["streams"].items() if s != 2})
    dg2, w2, c2, p2 = both(less, wire_of=(dg0, w0))
    assert c2["refused"] == 4 and c2["dgrams"] == 12 and p2["unknown_ssrc"] == 4 and p2["accepted"] == 12
    # the slot bound again, to a new SSRC and other payload types: the next call sees it
    new = dict(ses["streams"][2], ssrc=ses["streams"][2]["ssrc"] ^ 0x00FF00FF, pt=(101, 102))
    rtp.bind([2], new["ssrc"], new["ts_offset"], new["seq_offset"], new["pt"], level_id=2)
    again = dict(ses, streams={**less["streams"], 2: new})
    dg3, w3, c3, p3 = both(again)
    assert c3["dgrams"] == 16 and p3["accepted"] == 16
    _, _, _, p4 = both(again, wire_of=(dg0, w0))                  # the wire of the old binding: its SSRC is gone
    assert p4["unknown_ssrc"] == 4 and p4["accepted"] == 12
    # a level id of 0 for the session: parse finds no level, pack takes none
    rtp.bind([0], ses["streams"][0]["ssrc"], ses["streams"][0]["ts_offset"], ses["streams"][0]["seq_offset"], ses["streams"][0]["pt"], level_id=0)
    pc, _ = _check_parse(torch, rtp, batch, dict(again, level_id=0), play, dg3, w3)
    assert pc["accepted"] == 16 and pc["with_level"] == 0
    with pytest.raises(ValueError):
        rtp.pack(dev(torch, rec), dev(torch, np.array([16] + [0] * 7, np.int32)), dev(torch, pool), level=dev(torch, level))
    cnt = torch.zeros(8, dtype=torch.int32, device="cuda")
    r5, p5, l5 = dev(torch, rec), dev(torch, pool), dev(torch, level)
    assert rtp.lib.solo_rtp_pack(rtp.h, r5.data_ptr(), cnt.data_ptr(), 16, p5.data_ptr(), 400, l5.data_ptr(), 3, cnt.data_ptr(), cnt.data_ptr(), 0, cnt.data_ptr(),
                                 None) == -1
    # reset(): every stream unbound
    rtp.reset()
    pc, _ = _check_parse(torch, rtp, batch, dict(again, level_id=0, streams={}), play, dg3, w3)
    assert pc["unknown_ssrc"] == 16
    rtp.close()


# ---- capture: both halves of the tick, each a linear graph on one stream ---------------------------------------------------------------------------
def _fixture_session(level_id=3):
    rng = np.random.default_rng(99)
    return M.random_session(rng, 8, 640, level_id)


def test_capture_send_pack_and_rtp_pack(torch_cuda):
    """solo_send_pack and solo_rtp_pack behind it in one graph: the record count travels on the device.  Replays with other packets of the
    fixture and other levels equal the same calls made eagerly on a twin, and the model"""
    import solo_amd
    torch = torch_cuda
    z = G.fixture()
    P, SLOT, MAXR, WCAP = 3, z["bits"].shape[2], 48, 16384
    ses = _fixture_session()
    rng = np.random.default_rng(3)

    def make():
        h = solo_amd.SoloBatch(8, encoder=False, decoder=True, slot_bytes=SLOT)
        rtp = gpu_session(ses)
        ins = dict(bits=G.zeros(torch, (8, P, SLOT), torch.uint8), nbytes=G.zeros(torch, (8, P, 2), torch.int16), level=G.zeros(torch, (8, 4), torch.uint8))
        outs = dict(records=G.zeros(torch, (MAXR, 5), torch.int32), payload=G.zeros(torch, (8 * P * SLOT,), torch.uint8), scount=G.zeros(torch, (8,), torch.int32),
                    dgrams=G.zeros(torch, (MAXR, 2), torch.int32), wire=G.zeros(torch, (WCAP,), torch.uint8), count=G.zeros(torch, (8,), torch.int32))

        def call():
            r = h.lib.solo_send_pack(h.h, ins["bits"].data_ptr(), ins["nbytes"].data_ptr(), None, P, None, 500, outs["records"].data_ptr(), MAXR,
                                     outs["payload"].data_ptr(), 8 * P * SLOT, outs["scount"].data_ptr(), h._stream())
            return r or rtp.lib.solo_rtp_pack(rtp.h, outs["records"].data_ptr(), outs["scount"].data_ptr(), MAXR, outs["payload"].data_ptr(), 8 * P * SLOT,
                                              ins["level"].data_ptr(), 4, outs["dgrams"].data_ptr(), outs["wire"].data_ptr(), WCAP, outs["count"].data_ptr(),
                                              rtp._stream())
        return G.Stage(torch, ins, outs, call, keep=(h, rtp))

    feeds = [dict(bits=z["bits"][:, 3 * k:3 * k + 3], nbytes=z["nbytes"][:, 3 * k:3 * k + 3], level=rng.integers(0, 256, (8, 4), dtype=np.uint8)) for k in range(4)]

    def model(k, feed, got):
        n = int(got["scount"][0])
        want = M.model_pack(ses, got["records"], n, got["payload"], feed["level"], MAXR, WCAP)
        c = {f: int(v) for f, v in zip(("dgrams", "dgrams_needed"), got["count"][:2])}
        assert 0 < n <= MAXR and c["dgrams"] == c["dgrams_needed"] == want["count"]["dgrams"] == n, (k, n, c)
        assert int(got["count"][2:4].view(np.int64)[0]) == want["count"]["bytes"]
        assert np.array_equal(got["dgrams"][:n], want["dgrams"]) and np.array_equal(got["wire"][:want["count"]["bytes"]], want["wire"])
        assert (got["wire"][want["count"]["bytes"]:] == G.FILL).all() and (got["dgrams"][n:].view(np.uint8) == G.FILL).all()

    G.replay_against_twin(torch, make, feeds, model=model)


def test_capture_rtp_parse_and_recv_insert(torch_cuda):
    """solo_rtp_parse and solo_recv_insert behind it in one graph, a fixed capacity of 16 datagrams (a tick that brought fewer pads with
    {0, 0}: malformed, and `bad` to the ring): replay k files packet k of the fixture; afterwards the ring plays the reference decoder's PCM"""
    import solo_amd
    torch = torch_cuda
    z = G.fixture()
    pool, parts = G.datagrams()
    A, W, NP = 16, 8192, 4
    ses = _fixture_session()
    rng = np.random.default_rng(4)
    feeds, n_real = [], []
    for k in range(NP):
        dgs = []
        for (s, p, d), (off, ln) in sorted(parts.items()):
            if p == k:
                c = ses["streams"][s]
                dgs.append(M.build(c["ssrc"], c["pt"][d], 2 * k + d, c["ts_offset"] + k * 640, pool[off:off + ln].tobytes(), ext=M.level_ext(3, 16 * k + s)))
        dgs = [dgs[i] for i in rng.permutation(len(dgs))]
        table, wire = _lay_out(rng, dgs)
        dg = np.zeros((A, 2), np.int32)
        dg[:len(dgs)] = table
        w = np.zeros(W, np.uint8)
        w[:wire.size] = wire
        feeds.append(dict(dgrams=dg, wire=w))
        n_real.append(len(dgs))
    assert all(0 < v <= A for v in n_real) and any(v < A for v in n_real)

    def make():
        h = solo_amd.SoloBatch(8, encoder=False, decoder=True, slot_bytes=512)
        h.recv_create(8, 256, 0)
        rtp = gpu_session(ses)
        ins = dict(dgrams=G.zeros(torch, (A, 2), torch.int32), wire=G.zeros(torch, (W,), torch.uint8))
        outs = dict(arrivals=G.zeros(torch, (A, 5), torch.int32), level=G.zeros(torch, (A,), torch.uint8), rtp_seq=G.zeros(torch, (A,), torch.int16),
                    count=G.zeros(torch, (8,), torch.int32))

        def call():
            r = rtp.lib.solo_rtp_parse(rtp.h, h.h, ins["dgrams"].data_ptr(), A, ins["wire"].data_ptr(), W, outs["arrivals"].data_ptr(), outs["level"].data_ptr(),
                                       outs["rtp_seq"].data_ptr(), outs["count"].data_ptr(), rtp._stream())
            return r or h.lib.solo_recv_insert(h.h, outs["arrivals"].data_ptr(), A, ins["wire"].data_ptr(), W, h._stream())

        def state():
            s = h.recv_stats()
            return np.array([s[f] for f in ("inserted", "late", "ahead", "duplicate", "bad")], np.int64)
        return G.Stage(torch, ins, outs, call, state=state, keep=(h, rtp))

    play = np.zeros(8, np.int32)

    def model(k, feed, got):
        want = M.model_parse(ses, play, feed["dgrams"], feed["wire"])
        assert want["count"]["accepted"] == want["count"]["with_level"] == n_real[k] and want["count"]["malformed"] == A - n_real[k]
        assert got["count"].tolist() == [want["count"][f] for f in ("accepted", "with_level", "malformed", "version", "unknown_ssrc", "unknown_pt", "timestamp", "reserved")]
        assert np.array_equal(got["arrivals"], want["arrivals"]) and np.array_equal(got["level"], want["level"])
        assert np.array_equal(got["rtp_seq"].view(np.uint16), want["rtp_seq"])

    _, cap, twin = G.replay_against_twin(torch, make, feeds, model=model, stateful=True)
    assert cap.state().tolist() == [sum(n_real), 0, 0, 0, NP * A - sum(n_real)]
    for st in (cap, twin):
        pcm, status = st.keep[0].recv_decode(NP)
        assert int(host(torch, status).max()) == 0
        assert np.array_equal(host(torch, pcm), z["dec_loss"][:, :NP])

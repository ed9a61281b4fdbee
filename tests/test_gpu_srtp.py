"""The SRTP stage on the GPU (solo_srtp_protect / solo_srtp_unprotect through solo_amd.Rtp and the C ABI) against the independent model of
tests/srtp_model.py: protect over 1 and 257 records (one 256-record tile and a record) with the length, header, tag and wrap families of
tests/test_srtp_model.py, a stream without a tx key voided, and the records of a real solo_send_fanout; unprotect over 1 and 257
datagrams, the hostile set shuffled among valid ones at all four alignments, a second call continuing from the first call's index; the
secured chain encode -> send_pack -> rtp_pack -> srtp_protect -> network -> srtp_unprotect -> rtp_parse -> recv_insert -> recv_decode
bit for bit against the same chain in the clear; and both calls captured in a graph and replayed against eager twins.

CAPTURED names the test that captures each of the two calls the interface calls capturable (tests/test_srtp_model.py holds this file to it)."""
import numpy as np
import pytest

import graph_replay_lib as G
import rtp_model as R
import srtp_model as M
import solo_testlib as T
from test_gpu_rtp import dev, host, gpu_session, ring_handle

pytestmark = pytest.mark.gpu
CAPTURED = {"solo_srtp_protect": "test_capture_rtp_pack_and_srtp_protect", "solo_srtp_unprotect": "test_capture_srtp_unprotect_and_rtp_parse"}
FILL_D, FILL_W = -7, 0xA5


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch


def srtp_session(ses, roc0=None):
    """a solo_amd.Rtp bound and keyed as the model's session dict says (trailer = the largest tag)"""
    rtp = gpu_session(ses)
    tags = {k["tag"] for k in ses.get("srtp", {}).values()}
    rtp.set_trailer(max(tags) if tags else 0)
    for tag in sorted(tags):
        for d in ("tx", "rx"):
            ss = [s for s, k in sorted(ses["srtp"].items()) if k["tag"] == tag and k.get(d) is not None]
            if ss:
                rtp.set_keys(ss, tag_bytes=tag, rx_roc=None if d == "tx" or roc0 is None else [roc0.get(s, 0) for s in ss], **{d: [ses["srtp"][s][d] for s in ss]})
    return rtp


def cnt_of(rtp, count):
    c = rtp.srtp_count(count)
    return {k: c[k] for k in M.VERDICTS}


def want_cnt(want):
    return {k: want["count"][k] for k in M.VERDICTS}


# ---- protect ---------------------------------------------------------------------------------------------------------------------------------------------
def protect_records(rng, ses, n, with_level):
    """n records: the edge lengths, the wrap indices of streams 0 and 1, a stream without a tx key (4), an unbound one (5), a bad desc"""
    Hb = 20 if with_level else 12
    rec, at = [], 0
    special = [[0, 0, 0, 3, 40], [0, 0, 1, 5, 41], [0, 1, 0, 7, 42], [0, 1, 1, 9, 43], [1, 2 ** 31 - 1, 0, 11, 44], [1, 2 ** 31 - 1, 1, 13, 45], [4, 7, 0, 0, 30],
               [5, 7, 0, 0, 30], [2, 8, 2, 0, 30]]
    lens = M.edge_lengths(Hb)
    if n == 1:
        return np.array([[2, 100, 1, 0, 33]], np.int32), 400
    for i in range(n - len(special)):
        ln = lens[i % len(lens)] if i < 2 * len(lens) else int(rng.integers(1, 130))
        rec.append([int(rng.choice([0, 1, 2, 3, 4])), 100 + i, i % 2, at, ln])
        at += ln - 1
    order = rng.permutation(n)
    rec = np.array(rec + special, np.int32)[order]
    return rec, at + 400


@pytest.mark.parametrize("n", [1, 257])
@pytest.mark.parametrize("with_level,tag", [(False, 10), (True, 4)])
def test_protect_against_model(torch_cuda, n, with_level, tag):
    torch = torch_cuda
    rng = np.random.default_rng(900 + n + tag)
    ses = R.random_session(rng, 6, 640, 3, unbound=(5,))
    ses["streams"][0]["seq_offset"], ses["streams"][1]["seq_offset"] = 65534, 65535
    M.random_keys(rng, ses, tag, no_tx=(4,))
    rtp = srtp_session(ses)
    rec, pool_bytes = protect_records(rng, ses, n, with_level)
    pool = rng.integers(0, 256, pool_bytes, dtype=np.uint8)
    level = rng.integers(0, 255, (6, 4), dtype=np.uint8) if with_level else None
    sc = np.zeros(8, np.int32)
    sc[0] = n
    cap, GUARD = 4 * (pool_bytes + 40 * n), 64
    dg = torch.full((n + GUARD, 2), FILL_D, dtype=torch.int32, device="cuda")
    wire = torch.full((cap + GUARD,), FILL_W, dtype=torch.uint8, device="cuda")
    d_rec, d_sc = dev(torch, rec), dev(torch, sc)
    _, _, pc = rtp.pack(d_rec, d_sc, dev(torch, pool), level=None if level is None else dev(torch, level), dgrams=dg[:n], wire=wire[:cap])
    c = rtp.pack_count(pc)
    wp = M.model_pack_trailer(R, ses, rec, n, pool, level, tag)
    packed_dg, packed = host(torch, dg).copy(), host(torch, wire).copy()
    assert c == wp["count"] and np.array_equal(packed_dg[:n], wp["dgrams"]) and np.array_equal(packed[:c["bytes"]], wp["wire"])
    assert (packed[c["bytes"]:] == FILL_W).all()
    want = M.model_protect(ses, rec, n, packed_dg[:n], packed[:cap])
    count = rtp.protect(d_rec, d_sc, dg[:n], wire[:cap])
    got = cnt_of(rtp, count)
    print("srtp_protect %d records (H %d, tag %d): %s" % (n, 20 if with_level else 12, tag, got))
    assert got == want_cnt(want), (got, want["count"])
    hd, hw = host(torch, dg), host(torch, wire)
    assert np.array_equal(hd[:n], want["dgrams"]) and np.array_equal(hw[:cap], want["wire"])
    assert (hd[n:] == FILL_D).all() and (hw[cap:] == FILL_W).all() and (hw[c["bytes"]:cap] == FILL_W).all()
    if n > 1:
        assert got["no_key"] >= 1 and got["skipped"] == 2 and got["ok"] > 150 and got["malformed"] == 0
        k = int(np.nonzero(rec[:, 0] == 4)[0][0])
        assert tuple(hd[k]) == (0, 0) and tuple(packed_dg[k]) != (0, 0)
    # a refused list: ok = -1 and no datagram is touched; max_records cuts; host refusals of the C ABI
    d2, w2 = dev(torch, packed_dg[:n]), dev(torch, packed[:cap])
    bad_sc = dev(torch, np.array([-1] + [0] * 7, np.int32))
    count = rtp.protect(d_rec, bad_sc, d2, w2)
    assert cnt_of(rtp, count) == dict(dict.fromkeys(M.VERDICTS, 0), ok=-1) and np.array_equal(host(torch, d2), packed_dg[:n]) and np.array_equal(host(torch, w2), packed[:cap])
    L = rtp.lib
    a = lambda **k: [k.get("rec", d_rec.data_ptr()), k.get("sc", d_sc.data_ptr()), k.get("m", n), k.get("dg", d2.data_ptr()), k.get("wire", w2.data_ptr()),
                     k.get("wb", cap), k.get("cnt", count.data_ptr()), None]
    for bad in (dict(rec=None), dict(sc=None), dict(m=0), dict(m=-1), dict(dg=None), dict(wire=None), dict(wb=-1), dict(cnt=None), dict(dg=d2.data_ptr() + 2),
                dict(cnt=count.data_ptr() + 1), dict(rec=d_rec.data_ptr() + 1)):
        assert L.solo_srtp_protect(rtp.h, *a(**bad)) == -1, bad
    assert L.solo_srtp_protect(None, *a()) == -1
    torch.cuda.synchronize()
    assert np.array_equal(host(torch, d2), packed_dg[:n]) and np.array_equal(host(torch, w2), packed[:cap])
    rtp.close()


def test_protect_fanout_records(torch_cuda):
    """the records and the count of a real solo_send_fanout: 8 destinations share 2 sources' offsets, every destination's copy is packed
    and then protected under its own key"""
    import solo_amd
    torch = torch_cuda
    rng = np.random.default_rng(18)
    P, slot = 3, 128
    tx = solo_amd.SoloBatch(8, encoder=False, decoder=True, slot_bytes=slot)
    bits = rng.integers(0, 256, (2, P, slot), dtype=np.uint8)
    nb = np.zeros((2, P, 2), np.int16)
    nb[:, :, 0] = rng.integers(60, 120, (2, P))
    nb[:, :, 1] = nb[:, :, 0] // 2 - rng.integers(0, 9, (2, P))
    source = np.array([0, 1, 0, 1, 0, 1, 0, 1], np.int32)
    records, payload, scount = tx.send_fanout(dev(torch, bits), dev(torch, nb), dev(torch, source), first_seq=40)
    n = tx.send_count(scount)["records"]
    assert n == 48
    ses = M.random_keys(rng, R.random_session(rng, 8, 640, 0), 10)
    rtp = srtp_session(ses)
    wire = torch.full((16384,), FILL_W, dtype=torch.uint8, device="cuda")
    dg, w, cnt = rtp.pack(records, scount, payload, wire=wire)
    assert rtp.pack_count(cnt)["dgrams"] == 48
    rec, pdg, pw = host(torch, records), host(torch, dg).copy(), host(torch, w).copy()
    want = M.model_protect(ses, rec, n, pdg, pw)
    count = rtp.protect(records, scount, dg, w)
    assert cnt_of(rtp, count) == want_cnt(want) == dict(dict.fromkeys(M.VERDICTS, 0), ok=48)
    hd, hw = host(torch, dg), host(torch, w)
    assert np.array_equal(hd, want["dgrams"]) and np.array_equal(hw, want["wire"])
    # one source's packet under four keys: four different ciphertexts
    same = [k for k in range(n) if tuple(rec[k, 3:5]) == tuple(rec[0, 3:5])]
    assert len(same) == 4 and len({hw[hd[k, 0] + 12:hd[k, 0] + hd[k, 1] - 10].tobytes() for k in same}) == 4
    rtp.close()
    tx.close()


# ---- unprotect -------------------------------------------------------------------------------------------------------------------------------------------
def lay_out(rng, dgs):
    wire, table = bytearray(b"\x11" * 3), []
    for i, d in enumerate(dgs):
        wire += b"\x22" * int(rng.integers(0, 4))
        wire += b"\x22" * ((i - len(wire)) % 4 if i < 8 else 0)      # (the first eight: alignments 0, 1, 2, 3, 0, ... for certain)
        table.append((len(wire), len(d)))
        wire += d
    wire += b"\x33" * 16
    return np.array(table, np.int32).reshape(-1, 2), np.frombuffer(bytes(wire), np.uint8).copy()


def valid_packets(rng, ses, state, n):
    """n valid SRTP datagrams of the keyed streams: indices near each stream's receive state, distinct per stream"""
    out, used = [], {}
    keyed = [s for s, k in sorted(ses["srtp"].items()) if k.get("rx") is not None]
    while len(out) < n:
        s = int(rng.choice(keyed))
        st = state[s]
        base = st["index"] if st["index"] >= 0 else (st["roc0"] << 16) | 2000
        i = base + int(rng.integers(100, 3000))
        if i in used.setdefault(s, set()):
            continue
        used[s].add(i)
        c, k = ses["streams"][s], ses["srtp"][s]
        ext = R.level_ext(ses["level_id"], int(rng.integers(0, 255))) if rng.random() < 0.5 else None
        p = R.build(c["ssrc"], c["pt"][int(rng.integers(0, 2))], i & 0xFFFF, int(rng.integers(0, 2 ** 32)), rng.integers(0, 256, int(rng.integers(1, 120)), dtype=np.uint8).tobytes(),
                    ext=ext)
        out.append(M.protect_packet(M.session_keys(k["rx"]), k["tag"], p, i >> 16))
    return out


def check_unprotect(torch, rtp, ses, state, dg, wire):
    n = dg.shape[0]
    want = M.model_unprotect(ses, state, dg, wire)
    out = torch.full((n + 8, 2), FILL_D, dtype=torch.int32, device="cuda")
    backing = torch.full((wire.size + 128,), 0x3C, dtype=torch.uint8, device="cuda")
    w = backing[64:64 + wire.size]
    w.copy_(torch.from_numpy(wire))
    _, count = rtp.unprotect(dev(torch, dg), w, dgrams_out=out[:n])
    got = cnt_of(rtp, count)
    print("srtp_unprotect %d datagrams: %s" % (n, got))
    assert got == want_cnt(want), (got, want["count"])
    ho, hb = host(torch, out), host(torch, backing)
    assert np.array_equal(ho[:n], want["dgrams"]) and (ho[n:] == FILL_D).all()
    assert np.array_equal(hb[64:64 + wire.size], want["wire"]) and (hb[:64] == 0x3C).all() and (hb[64 + wire.size:] == 0x3C).all()
    assert rtp.rx_index() == [want["state"][s]["index"] for s in range(ses["n_streams"])]
    return want


@pytest.mark.parametrize("n,tag", [(1, 10), (257, 10), (257, 4)])
def test_unprotect_against_model(torch_cuda, n, tag):
    torch = torch_cuda
    rng = np.random.default_rng(950 + n + tag)
    ses = R.random_session(rng, 6, 640, 5, unbound=(3,))
    M.random_keys(rng, ses, tag, no_rx=(4,))
    roc0 = {0: 0, 1: 65535, 2: 7, 5: 2 ** 32 - 1}
    state = M.new_state(ses, roc0)
    rtp = srtp_session(ses, roc0)
    for call in range(2):                                             # the second call continues from the first call's index
        dgs = []
        if n > 1:
            kinds = M.hostile_set(ses, state, 2, rng, R) + M.hostile_set(ses, state, 0, rng, R)
            c4 = ses["streams"][4]
            dgs = [k[1] for k in kinds] + [R.build(c4["ssrc"], 96, 3, 0, b"x" * 30)]
        dgs += valid_packets(rng, ses, state, n - len(dgs))
        if call == 1 and n > 1:                                       # a replay of the first call's datagram authenticates again: the ring is the judge
            dgs[-1] = first
        first = dgs[-1]
        dgs = [dgs[i] for i in rng.permutation(n)]
        dg, wire = lay_out(rng, dgs)
        if n > 1:
            assert {int(v) for v in dg[:, 0] % 4} == {0, 1, 2, 3}
            dg = np.concatenate([dg, np.array([[-1, 40], [wire.size - 39, 40], [wire.size, 16], [2 ** 31 - 1, 2 ** 31 - 1], [0, -5]], np.int32)])
        want = check_unprotect(torch, rtp, ses, state, dg, wire)
        if n > 1:
            assert all(want["count"][v] > 0 for v in ("ok", "malformed", "unknown_ssrc", "no_key", "auth_failed")) and want["count"]["ok"] > 150
        state = want["state"]
    assert any(v["index"] >= 0 for v in state.values())
    # host refusals of the C ABI
    L = rtp.lib
    d5, w5 = dev(torch, dg), dev(torch, wire)
    o5 = torch.zeros((dg.shape[0], 2), dtype=torch.int32, device="cuda")
    cnt = torch.zeros(8, dtype=torch.int32, device="cuda")
    a = lambda **k: [k.get("dg", d5.data_ptr()), k.get("n", dg.shape[0]), k.get("wire", w5.data_ptr()), k.get("wb", wire.size), k.get("out", o5.data_ptr()),
                     k.get("cnt", cnt.data_ptr()), None]
    for bad in (dict(dg=None), dict(n=-1), dict(wire=None), dict(wb=-1), dict(out=None), dict(cnt=None), dict(dg=d5.data_ptr() + 2), dict(out=o5.data_ptr() + 1)):
        assert L.solo_srtp_unprotect(rtp.h, *a(**bad)) == -1, bad
    assert L.solo_srtp_unprotect(None, *a()) == -1
    before = rtp.rx_index()
    _, c0 = rtp.unprotect(d5[:0], w5)                                 # no datagram: the count is cleared, nothing else happens
    assert cnt_of(rtp, c0) == dict.fromkeys(M.VERDICTS, 0) and rtp.rx_index() == before
    # clear_keys and unbind on the device
    rtp.clear_keys([2])
    assert rtp.rx_index([2]) == [-1]
    rtp.unbind([0])
    assert rtp.rx_index([0]) == [-1]
    with pytest.raises(RuntimeError):
        rtp.set_trailer(0)                                            # (streams 1 and 5 still hold tx keys)
    rtp.close()


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------------------
def test_end_to_end(torch_cuda):
    """8 streams x 3 packets of the fixture: encode -> send_pack -> rtp_pack (trailer 10) -> srtp_protect -> shuffle, drop every fifth,
    tamper two -> srtp_unprotect -> rtp_parse -> recv_insert -> recv_decode gives PCM and status bit for bit equal to the same chain without
    SRTP, in which the tampered datagrams are dropped"""
    import solo_amd
    torch = torch_cuda
    z = G.fixture()
    rng = np.random.default_rng(77)
    N, P, S, FIRST = 8, 3, z["bits"].shape[2], 500
    enc = solo_amd.SoloBatch(N, encoder=True, decoder=False, slot_bytes=S)
    bits, nb, st = enc.encode(dev(torch, z["pcm"][:, :P]))
    torch.cuda.synchronize()
    assert int(st.abs().max()) == 0 and np.array_equal(host(torch, nb), z["nbytes"][:, :P])
    ses = M.random_keys(rng, R.random_session(rng, N, 640, 2), 10)
    for s, c in ses["streams"].items():                               # odd streams send under rollover counter 1, even ones under 0
        c["seq_offset"] = 65000 if s % 2 else c["seq_offset"] % 30000
    for k in ses["srtp"].values():
        k["rx"] = k["tx"]
    roc0 = {s: ((ses["streams"][s]["seq_offset"] + 2 * FIRST) >> 16) for s in range(N)}
    level = rng.integers(0, 255, (N, P), dtype=np.uint8)

    def chain(secure):
        rtp = srtp_session(ses if secure else dict(ses, srtp={}), roc0)
        rtp.set_trailer(10)
        records, payload, scount = enc.send_pack(bits, nb, first_seq=FIRST)
        n = enc.send_count(scount)["records"]
        dgrams, wire, cnt = rtp.pack(records, scount, payload, level=dev(torch, level))
        assert rtp.pack_count(cnt)["dgrams"] == n == 2 * N * P
        if secure:
            assert cnt_of(rtp, rtp.protect(records, scount, dgrams, wire))["ok"] == n
        return rtp, n, host(torch, dgrams)[:n].copy(), wire

    rtp, n, dg, wire = chain(True)
    clear_rtp, n2, dg2, wire2 = chain(False)
    assert n2 == n and np.array_equal(dg2[:, 0], dg[:, 0]) and np.array_equal(dg2[:, 1] + 10, dg[:, 1])
    hw, hw2 = host(torch, wire), host(torch, wire2)
    assert np.array_equal(hw[dg[0, 0]:dg[0, 0] + 20], hw2[dg[0, 0]:dg[0, 0] + 20]) and not np.array_equal(hw[dg[0, 0] + 20:dg[0, 0] + 60], hw2[dg[0, 0] + 20:dg[0, 0] + 60])
    assert sorted(set(roc0.values())) == [0, 1]
    # the network: another order, every fifth datagram lost, two tampered (a payload bit, a tag bit)
    perm = rng.permutation(n)
    keep = np.array([perm[i] for i in range(n) if i % 5 != 4])
    t1, t2 = int(keep[3]), int(keep[11])
    wire[int(dg[t1, 0]) + 30] ^= 0x04
    wire[int(dg[t2, 0] + dg[t2, 1]) - 1] ^= 0x80
    out, ucnt = rtp.unprotect(dev(torch, dg[keep]), wire)
    assert cnt_of(rtp, ucnt) == dict(dict.fromkeys(M.VERDICTS, 0), ok=len(keep) - 2, auth_failed=2)
    rx = ring_handle(N, [FIRST] * N, depth=P)
    arr, lv, sq, pcnt = rtp.parse(rx, out, wire, level=True)
    pc = rtp.parse_count(pcnt)
    assert pc["accepted"] == pc["with_level"] == len(keep) - 2 and pc["malformed"] == 2
    rx.recv_insert(arr, wire)
    assert rx.recv_stats() == dict(inserted=len(keep) - 2, late=0, ahead=0, duplicate=0, bad=2)
    got, st = rx.recv_decode(P)
    # the same chain in the clear, the tampered datagrams dropped
    keep2 = np.array([k for k in keep if k not in (t1, t2)])
    raw = ring_handle(N, [FIRST] * N, depth=P)
    arr2, lv2, _, pcnt2 = clear_rtp.parse(raw, dev(torch, dg2[keep2]), wire2, level=True)
    assert clear_rtp.parse_count(pcnt2)["accepted"] == len(keep2)
    raw.recv_insert(arr2, wire2)
    want, st2 = raw.recv_decode(P)
    assert np.array_equal(host(torch, got), host(torch, want)) and np.array_equal(host(torch, st), host(torch, st2)) and host(torch, got).any()
    ok_rows = host(torch, arr)[:, 0] >= 0
    assert np.array_equal(host(torch, lv)[ok_rows], host(torch, lv2))
    rtp.close()
    clear_rtp.close()


# ---- capture ---------------------------------------------------------------------------------------------------------------------------------------------
def _fixture_session():
    rng = np.random.default_rng(98)
    ses = M.random_keys(rng, R.random_session(rng, 8, 640, 3), 10)
    for k in ses["srtp"].values():
        k["rx"] = k["tx"]
    return ses


def test_capture_rtp_pack_and_srtp_protect(torch_cuda):
    """solo_send_pack, solo_rtp_pack and solo_srtp_protect behind it in one graph: the record count travels on the device.  Replays with
    other packets of the fixture equal the same calls made eagerly on a twin, and the model"""
    import solo_amd
    torch = torch_cuda
    z = G.fixture()
    P, SLOT, MAXR, WCAP = 3, z["bits"].shape[2], 48, 16384
    ses = _fixture_session()
    rng = np.random.default_rng(3)

    def make():
        h = solo_amd.SoloBatch(8, encoder=False, decoder=True, slot_bytes=SLOT)
        rtp = srtp_session(ses)
        ins = dict(bits=G.zeros(torch, (8, P, SLOT), torch.uint8), nbytes=G.zeros(torch, (8, P, 2), torch.int16), level=G.zeros(torch, (8, 4), torch.uint8))
        outs = dict(records=G.zeros(torch, (MAXR, 5), torch.int32), payload=G.zeros(torch, (8 * P * SLOT,), torch.uint8), scount=G.zeros(torch, (8,), torch.int32),
                    dgrams=G.zeros(torch, (MAXR, 2), torch.int32), wire=G.zeros(torch, (WCAP,), torch.uint8), count=G.zeros(torch, (8,), torch.int32),
                    scnt=G.zeros(torch, (8,), torch.int32))

        def call():
            r = h.lib.solo_send_pack(h.h, ins["bits"].data_ptr(), ins["nbytes"].data_ptr(), None, P, None, 500, outs["records"].data_ptr(), MAXR,
                                     outs["payload"].data_ptr(), 8 * P * SLOT, outs["scount"].data_ptr(), h._stream())
            r = r or rtp.lib.solo_rtp_pack(rtp.h, outs["records"].data_ptr(), outs["scount"].data_ptr(), MAXR, outs["payload"].data_ptr(), 8 * P * SLOT,
                                           ins["level"].data_ptr(), 4, outs["dgrams"].data_ptr(), outs["wire"].data_ptr(), WCAP, outs["count"].data_ptr(), rtp._stream())
            return r or rtp.lib.solo_srtp_protect(rtp.h, outs["records"].data_ptr(), outs["scount"].data_ptr(), MAXR, outs["dgrams"].data_ptr(), outs["wire"].data_ptr(),
                                                  WCAP, outs["scnt"].data_ptr(), rtp._stream())
        return G.Stage(torch, ins, outs, call, keep=(h, rtp))

    feeds = [dict(bits=z["bits"][:, 3 * k:3 * k + 3], nbytes=z["nbytes"][:, 3 * k:3 * k + 3], level=rng.integers(0, 255, (8, 4), dtype=np.uint8)) for k in range(4)]

    def model(k, feed, got):
        n = int(got["scount"][0])
        wp = M.model_pack_trailer(R, ses, got["records"], n, got["payload"], feed["level"], 10, MAXR, WCAP)
        want = M.model_protect(ses, got["records"], n, wp["dgrams"], np.concatenate([wp["wire"], np.zeros(64, np.uint8)]), MAXR)
        assert 0 < n <= MAXR and got["scnt"].tolist() == [n, 0, 0, 0, 0, 0, 0, 0], (k, n, got["scnt"])
        nb = wp["count"]["bytes"]
        assert np.array_equal(got["dgrams"][:n], want["dgrams"][:n]) and np.array_equal(got["wire"][:nb], want["wire"][:nb])
        assert (got["wire"][nb:] == G.FILL).all() and (got["dgrams"][n:].view(np.uint8) == G.FILL).all()

    G.replay_against_twin(torch, make, feeds, model=model)


def test_capture_srtp_unprotect_and_rtp_parse(torch_cuda):
    """solo_srtp_unprotect, solo_rtp_parse and solo_recv_insert behind it in one graph, a fixed capacity of 16 datagrams: replay k files
    packet k of the fixture, protected by the model; captured stage and eager twin start from the same receive state and end in the same;
    afterwards the ring plays the reference decoder's PCM"""
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
                i = 65534 + 2 * k + d                                 # the rollover counter moves inside the run
                rtpp = R.build(c["ssrc"], c["pt"][d], i & 0xFFFF, c["ts_offset"] + k * 640, pool[off:off + ln].tobytes(), ext=R.level_ext(3, 16 * k + s))
                dgs.append(M.protect_packet(M.session_keys(ses["srtp"][s]["rx"]), 10, rtpp, i >> 16))
        dgs = [dgs[i] for i in rng.permutation(len(dgs))]
        table, wire = lay_out(rng, dgs)
        dg = np.zeros((A, 2), np.int32)
        dg[:len(dgs)] = table
        w = np.zeros(W, np.uint8)
        w[:wire.size] = wire
        feeds.append(dict(dgrams=dg, wire=w))
        n_real.append(len(dgs))
    assert all(0 < v <= A for v in n_real)

    def make():
        h = solo_amd.SoloBatch(8, encoder=False, decoder=True, slot_bytes=512)
        h.recv_create(8, 256, 0)
        rtp = srtp_session(ses)
        ins = dict(dgrams=G.zeros(torch, (A, 2), torch.int32), wire=G.zeros(torch, (W,), torch.uint8))
        outs = dict(rtp_dgrams=G.zeros(torch, (A, 2), torch.int32), scnt=G.zeros(torch, (8,), torch.int32), arrivals=G.zeros(torch, (A, 5), torch.int32),
                    level=G.zeros(torch, (A,), torch.uint8), count=G.zeros(torch, (8,), torch.int32))

        def call():
            r = rtp.lib.solo_srtp_unprotect(rtp.h, ins["dgrams"].data_ptr(), A, ins["wire"].data_ptr(), W, outs["rtp_dgrams"].data_ptr(), outs["scnt"].data_ptr(),
                                            rtp._stream())
            r = r or rtp.lib.solo_rtp_parse(rtp.h, h.h, outs["rtp_dgrams"].data_ptr(), A, ins["wire"].data_ptr(), W, outs["arrivals"].data_ptr(),
                                            outs["level"].data_ptr(), None, outs["count"].data_ptr(), rtp._stream())
            return r or h.lib.solo_recv_insert(h.h, outs["arrivals"].data_ptr(), A, ins["wire"].data_ptr(), W, h._stream())

        def state():
            s = h.recv_stats()
            return np.array([s[f] for f in ("inserted", "late", "ahead", "duplicate", "bad")] + rtp.rx_index(), np.int64)
        return G.Stage(torch, ins, outs, call, state=state, keep=(h, rtp))

    st = {"s": M.new_state(ses)}

    def model(k, feed, got):
        want = M.model_unprotect(ses, st["s"], feed["dgrams"], feed["wire"])
        st["s"] = want["state"]
        assert want["count"]["ok"] == n_real[k] and want["count"]["malformed"] == A - n_real[k]
        assert got["scnt"].tolist()[:6] == [want["count"][v] for v in M.VERDICTS] and np.array_equal(got["rtp_dgrams"], want["dgrams"])
        assert got["count"][0] == n_real[k] == got["count"][1] and got["count"][2] == A - n_real[k]

    _, cap, twin = G.replay_against_twin(torch, make, feeds, model=model, stateful=True)
    assert cap.state().tolist()[:5] == [sum(n_real), 0, 0, 0, NP * A - sum(n_real)]
    assert cap.state().tolist()[5:] == [st["s"][s]["index"] for s in range(8)] and max(cap.state().tolist()[5:]) >= 65536
    for s in (cap, twin):
        pcm, status = s.keep[0].recv_decode(NP)
        assert int(host(torch, status).max()) == 0
        assert np.array_equal(host(torch, pcm), z["dec_loss"][:, :NP])

"""AEAD_AES_128_GCM in the SRTP and the SRTCP stage on the GPU (RFC 7714; the four device calls through solo_amd.Rtp and the C ABI with keys
set by solo_srtp_set_keys_gcm / solo_srtcp_set_keys_gcm) against the independent model of tests/srtp_gcm_model.py, byte for byte.  The GCM
kernels take a tile of 64 datagrams, so the shapes are 1 and 65 (a tile and one), and 130 where the hostile sets alone fill more than a
tile.  Sessions hold AES-CM / HMAC streams, a keyless and an unbound stream beside the GCM ones: every datagram is counted once.

CAPTURED names the test that captures each of the four device calls with GCM keys (tests/test_srtp_gcm_model.py holds this file and the
header's block to it)."""
import copy
import os

import numpy as np
import pytest

import graph_replay_lib as GR
import rtcp_model as RC
import rtp_model as R
import solo_testlib as T
import srtcp_model as CM
import srtp_gcm_model as G
import srtp_model as S
import test_gpu_srtcp as GC
import test_srtcp_model as CPUC
import test_srtp_gcm_model as CPU
from test_gpu_rtp import dev, host, gpu_session, ring_handle

pytestmark = pytest.mark.gpu
CAPTURED = {"solo_srtp_protect": "test_capture_srtp_gcm_protect_and_unprotect", "solo_srtp_unprotect": "test_capture_srtp_gcm_protect_and_unprotect",
            "solo_srtcp_protect": "test_capture_srtcp_gcm_protect_and_unprotect", "solo_srtcp_unprotect": "test_capture_srtcp_gcm_protect_and_unprotect"}
FILL_D, FILL_W = -7, 0xA5
TILE = 64
ZERO = dict.fromkeys(CM.VERDICTS, 0)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch


def srtp_session(ses, roc0=None):
    """a solo_amd.Rtp bound and keyed as the model's session dict says: a GCM entry through set_keys_gcm (trailer = the largest tag)"""
    rtp = gpu_session(ses)
    tags = {k["tag"] for k in ses.get("srtp", {}).values()}
    rtp.set_trailer(max(tags) if tags else 0)
    for tag in sorted(tags):
        for d in ("tx", "rx"):
            ss = [s for s, k in sorted(ses["srtp"].items()) if k["tag"] == tag and k.get(d) is not None]
            if ss:
                kw = dict(rx_roc=None if d == "tx" or roc0 is None else [roc0.get(s, 0) for s in ss], **{d: [ses["srtp"][s][d] for s in ss]})
                rtp.set_keys_gcm(ss, **kw) if tag == G.TAG else rtp.set_keys(ss, tag_bytes=tag, **kw)
    return rtp


def cnt_of(rtp, count):
    c = rtp.srtp_count(count)
    return {k: c[k] for k in S.VERDICTS}


def want_cnt(want):
    return {k: want["count"][k] for k in S.VERDICTS}


# ---- SRTP protect -----------------------------------------------------------------------------------------------------------------------------------------
def protect_records(rng, n):
    """n records over the mixed session of the CPU test: every plaintext length (257 and 300: a row's lanes take a second keystream block,
    GHASH runs more than 16 blocks), the wrap indices of the GCM streams 0 and 1, the keyless stream 4, the unbound 5, a bad desc"""
    if n == 1:
        return np.array([[1, 100, 1, 0, 33]], np.int32), 400
    special = [[0, 0, 0, 3, 40], [0, 0, 1, 5, 41], [0, 1, 0, 7, 42], [1, 2 ** 31 - 1, 0, 11, 44], [1, 2 ** 31 - 1, 1, 13, 45], [4, 7, 0, 0, 30], [5, 7, 0, 0, 30], [0, 8, 2, 0, 30]]
    rec, at, lens = [], 0, G.LENGTHS[1:]
    for i in range(n - len(special)):
        ln = lens[i % len(lens)] if i < 3 * len(lens) else int(rng.integers(1, 130))
        rec.append([[0, 1, 2, 0, 3, 1][i % 6] if i < 3 * len(lens) else int(rng.choice([0, 1, 2, 3, 4])), 100 + i, i % 2, at, ln])
        at += ln - 1
    return np.array(rec + special, np.int32)[rng.permutation(n)], at + 400


@pytest.mark.parametrize("n", [1, TILE + 1])
@pytest.mark.parametrize("with_level", [False, True])
def test_srtp_protect_against_model(torch_cuda, n, with_level):
    torch = torch_cuda
    rng = np.random.default_rng(1900 + n + with_level)
    ses = CPU.mixed_session(rng, 3)
    ses["streams"][0]["seq_offset"], ses["streams"][1]["seq_offset"] = 65534, 65535
    rtp = srtp_session(ses)
    rec, pool_bytes = protect_records(rng, n)
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
    wp = S.model_pack_trailer(R, ses, rec, n, pool, level, 16)
    packed_dg, packed = host(torch, dg).copy(), host(torch, wire).copy()
    assert c == wp["count"] and np.array_equal(packed_dg[:n], wp["dgrams"]) and np.array_equal(packed[:c["bytes"]], wp["wire"])
    want = G.model_protect(ses, rec, n, packed_dg[:n], packed[:cap])
    count = rtp.protect(d_rec, d_sc, dg[:n], wire[:cap])
    got = cnt_of(rtp, count)
    print("srtp_protect (GCM and AES-CM streams) %d records, H %d: %s" % (n, 20 if with_level else 12, got))
    assert got == want_cnt(want), (got, want["count"])
    assert sum(got.values()) == n and host(torch, count)[6:].tolist() == [0, 0]                     # every datagram counted once
    hd, hw = host(torch, dg), host(torch, wire)
    assert np.array_equal(hd[:n], want["dgrams"]) and np.array_equal(hw[:cap], want["wire"])
    assert (hd[n:] == FILL_D).all() and (hw[cap:] == FILL_W).all() and (hw[c["bytes"]:cap] == FILL_W).all()
    if n > 1:
        assert got["no_key"] >= 1 and got["skipped"] == 2 and got["ok"] == n - 2 - got["no_key"] and got["malformed"] == 0
        grown = {int(s): set((hd[:n, 1] - packed_dg[:n, 1])[(rec[:, 0] == s) & (hd[:n, 1] > 0)].tolist()) for s in range(4)}
        assert grown == {0: {16}, 1: {16}, 2: {10}, 3: {4}}
    # a refused list: ok = -1 and no datagram is touched; max_records cuts
    d2, w2 = dev(torch, packed_dg[:n]), dev(torch, packed[:cap])
    bad_sc = dev(torch, np.array([-1] + [0] * 7, np.int32))
    count = rtp.protect(d_rec, bad_sc, d2, w2)
    assert cnt_of(rtp, count) == dict(dict.fromkeys(S.VERDICTS, 0), ok=-1) and np.array_equal(host(torch, d2), packed_dg[:n]) and np.array_equal(host(torch, w2), packed[:cap])
    if n > 1:
        m = 40
        cut = G.model_protect(ses, rec, n, packed_dg[:n], packed[:cap], max_records=m)
        count = rtp.protect(d_rec[:m], d_sc, d2[:m], w2)
        assert cnt_of(rtp, count) == want_cnt(cut) and np.array_equal(host(torch, d2), cut["dgrams"]) and np.array_equal(host(torch, w2), cut["wire"])
    rtp.close()


# ---- SRTP unprotect ---------------------------------------------------------------------------------------------------------------------------------------
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
    """n valid datagrams of the keyed streams, GCM or AES-CM as the stream's key says: indices near each stream's state, distinct per stream"""
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
        p = R.build(c["ssrc"], c["pt"][int(rng.integers(0, 2))], i & 0xFFFF, int(rng.integers(0, 2 ** 32)), rng.integers(0, 256, int(rng.integers(0, 320)), dtype=np.uint8).tobytes(),
                    ext=ext)
        out.append(G.protect_packet(G.session_keys(k["rx"]), p, i >> 16) if k.get("gcm") else S.protect_packet(S.session_keys(k["rx"]), k["tag"], p, i >> 16))
    return out


@pytest.mark.parametrize("n", [1, 2 * TILE + 2])
def test_srtp_unprotect_against_model(torch_cuda, n):
    torch = torch_cuda
    rng = np.random.default_rng(1950 + n)
    ses = CPU.mixed_session(rng, 5)
    ses["srtp"][4] = dict(G.gcm_entry(rng), rx=None)
    roc0 = {0: 7, 1: 65535, 2: 0, 3: 2 ** 32 - 1}
    state = S.new_state(ses, roc0)
    rtp = srtp_session(ses, roc0)
    for call in range(2):                                             # the second call continues from the first call's index
        dgs = []
        if n > 1:
            kinds = G.hostile_set(ses, state, 0, rng, R) + G.hostile_set(ses, state, 1, rng, R) + S.hostile_set(ses, state, 2, rng, R)
            dgs = [k[1] for k in kinds] + [R.build(ses["streams"][4]["ssrc"], 96, 3, 0, b"x" * 30)]
            assert len(dgs) >= TILE                                  # (the hostile sets alone fill a tile: the call takes three)
        dgs += valid_packets(rng, ses, state, n - len(dgs) - (5 if n > 1 else 0))
        dgs = [dgs[i] for i in rng.permutation(len(dgs))]
        dg, wire = lay_out(rng, dgs)
        if n > 1:
            assert {int(v) for v in dg[:, 0] % 4} == {0, 1, 2, 3}
            dg = np.concatenate([dg, np.array([[-1, 40], [wire.size - 39, 40], [wire.size, 16], [2 ** 31 - 1, 2 ** 31 - 1], [0, -5]], np.int32)])
        assert dg.shape[0] == n
        want = G.model_unprotect(ses, state, dg, wire)
        out = torch.full((n + 8, 2), FILL_D, dtype=torch.int32, device="cuda")
        backing = torch.full((wire.size + 128,), 0x3C, dtype=torch.uint8, device="cuda")
        w = backing[64:64 + wire.size]
        w.copy_(torch.from_numpy(wire))
        _, count = rtp.unprotect(dev(torch, dg), w, dgrams_out=out[:n])
        got = cnt_of(rtp, count)
        print("srtp_unprotect (GCM and AES-CM streams) %d datagrams: %s" % (n, got))
        assert got == want_cnt(want), (got, want["count"])
        assert sum(got.values()) == n and host(torch, count)[6:].tolist() == [0, 0]
        ho, hb = host(torch, out), host(torch, backing)
        assert np.array_equal(ho[:n], want["dgrams"]) and (ho[n:] == FILL_D).all()
        assert np.array_equal(hb[64:64 + wire.size], want["wire"]) and (hb[:64] == 0x3C).all() and (hb[64 + wire.size:] == 0x3C).all()
        for (off, ln), v in zip(dg.tolist(), want["verdicts"]):        # a rejected datagram keeps every byte
            if v != "ok" and off >= 0 and ln >= 0 and off + ln <= wire.size:
                assert np.array_equal(hb[64 + off:64 + off + ln], wire[off:off + ln])
        assert rtp.rx_index() == [want["state"][s]["index"] for s in range(6)]
        if n > 1:
            assert all(want["count"][v] > 0 for v in ("ok", "malformed", "unknown_ssrc", "no_key", "auth_failed")) and want["count"]["ok"] > 40
        if n > 1 and call == 0:                                       # into the list itself: d_dgrams_out may be d_dgrams
            twin = srtp_session(ses, roc0)
            d2, w2 = dev(torch, dg), dev(torch, wire)
            _, c2 = twin.unprotect(d2, w2, dgrams_out=d2)
            assert cnt_of(twin, c2) == want_cnt(want) and np.array_equal(host(torch, d2), want["dgrams"]) and np.array_equal(host(torch, w2), want["wire"])
            twin.close()
        state = want["state"]
    assert any(v["index"] >= 0 for v in state.values())
    rtp.close()


def test_fixture_datagrams(torch_cuda):
    """The fixture's RTP packets (tests/golden/srtp_gcm_cases.npz) with their SSRCs, sequence numbers and rollover counters.  The C ABI takes
    master keys, not session keys, so the fixture's libcrypto-made datagrams cannot be fed to the device under their own keys; the
    comparison goes by masters instead: tests/test_srtp_gcm_model.py pins the model to libcrypto on exactly these packets and lengths (and
    the host form, which runs the kernels' per-datagram source, to the fixture's bytes under the fixture's session keys); here the device
    is pinned to the model on the same packets under keys derived from random masters -- accepted and decrypted to the fixture's
    plaintext, and protecting the plaintext reproduces the model's datagram byte for byte."""
    torch = torch_cuda
    z = np.load(os.path.join(T.GOLDEN, "srtp_gcm_cases.npz"))
    off, meta = z["srtp_plain_off"], z["srtp_meta"].tolist()
    plain = [z["srtp_plain_blob"][off[i]:off[i + 1]].tobytes() for i in range(len(meta))]
    rng = np.random.default_rng(61)
    n = len(meta)
    ses = R.session(n, 640, 3, {s: dict(ssrc=int(m[0]), ts_offset=0, seq_offset=int(m[2]), pt=(96, 97)) for s, m in enumerate(meta)})
    ses["srtp"] = {s: G.gcm_entry(rng) for s in range(n)}
    for k in ses["srtp"].values():
        k["rx"] = k["tx"]
    roc0 = {s: int(m[1]) for s, m in enumerate(meta)}
    rtp = srtp_session(ses, roc0)
    wires = [G.protect_packet(G.session_keys(ses["srtp"][s]["rx"]), plain[s], roc0[s]) for s in range(n)]
    dg, wire = lay_out(rng, wires)
    d_w = dev(torch, wire)
    out, count = rtp.unprotect(dev(torch, dg), d_w)
    assert cnt_of(rtp, count) == dict(dict.fromkeys(S.VERDICTS, 0), ok=n)
    hw, ho = host(torch, d_w), host(torch, out)
    for s in range(n):
        assert hw[ho[s, 0]:ho[s, 0] + ho[s, 1]].tobytes() == plain[s], s
    assert rtp.rx_index() == [(roc0[s] << 16) | int(meta[s][2]) for s in range(n)]
    # protect: record s = (stream s, seq, desc 0) with seq_offset + 2 seq = the packet's index, for the counters an int32 seq reaches
    sel = [s for s in range(n) if roc0[s] < 2 ** 15]
    assert len(sel) >= 6
    rec = np.array([[s, (roc0[s] << 16) // 2, 0, 0, len(plain[s]) - int(meta[s][3])] for s in sel], np.int32)
    dg, wire = lay_out(rng, [plain[s] + bytes(19) for s in sel])
    dg[:, 1] -= 19
    d_dg, d_w = dev(torch, dg), dev(torch, wire)
    sc = np.zeros(8, np.int32)
    sc[0] = len(sel)
    count = rtp.protect(dev(torch, rec), dev(torch, sc), d_dg, d_w)
    assert cnt_of(rtp, count) == dict(dict.fromkeys(S.VERDICTS, 0), ok=len(sel))
    hw, hd = host(torch, d_w), host(torch, d_dg)
    for (o, ln), s in zip(hd.tolist(), sel):
        assert hw[o:o + ln].tobytes() == wires[s], s
    rtp.close()


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------------------
def test_secured_chain_equals_the_chain_in_the_clear(torch_cuda):
    """8 streams x 2 packets of the codec fixture: encode -> send_pack -> rtp_pack (trailer 16) -> srtp_protect -> shuffle, drop every fifth,
    tamper two -> srtp_unprotect -> rtp_parse -> recv_insert -> recv_decode under GCM keys gives PCM and status bit for bit equal to the
    same chain without SRTP, in which the tampered datagrams are dropped"""
    import solo_amd
    torch = torch_cuda
    z = GR.fixture()
    rng = np.random.default_rng(177)
    N, P, SLOT, FIRST = 8, 2, z["bits"].shape[2], 500
    enc = solo_amd.SoloBatch(N, encoder=True, decoder=False, slot_bytes=SLOT)
    bits, nb, st = enc.encode(dev(torch, z["pcm"][:, :P]))
    torch.cuda.synchronize()
    assert int(st.abs().max()) == 0 and np.array_equal(host(torch, nb), z["nbytes"][:, :P])
    ses = R.random_session(rng, N, 640, 2)
    ses["srtp"] = {s: G.gcm_entry(rng) for s in range(N)}
    for s, c in ses["streams"].items():                               # odd streams send under rollover counter 1, even ones under 0
        c["seq_offset"] = 65000 if s % 2 else c["seq_offset"] % 30000
    for k in ses["srtp"].values():
        k["rx"] = k["tx"]
    roc0 = {s: ((ses["streams"][s]["seq_offset"] + 2 * FIRST) >> 16) for s in range(N)}
    level = rng.integers(0, 255, (N, P), dtype=np.uint8)

    def chain(secure):
        rtp = srtp_session(ses if secure else dict(ses, srtp={}), roc0)
        rtp.set_trailer(16)
        records, payload, scount = enc.send_pack(bits, nb, first_seq=FIRST)
        n = enc.send_count(scount)["records"]
        dgrams, wire, cnt = rtp.pack(records, scount, payload, level=dev(torch, level))
        assert rtp.pack_count(cnt)["dgrams"] == n == 2 * N * P
        if secure:
            assert cnt_of(rtp, rtp.protect(records, scount, dgrams, wire))["ok"] == n
        return rtp, n, host(torch, dgrams)[:n].copy(), wire

    rtp, n, dg, wire = chain(True)
    clear_rtp, n2, dg2, wire2 = chain(False)
    assert n2 == n and np.array_equal(dg2[:, 0], dg[:, 0]) and np.array_equal(dg2[:, 1] + 16, dg[:, 1])
    hw, hw2 = host(torch, wire), host(torch, wire2)
    assert np.array_equal(hw[dg[0, 0]:dg[0, 0] + 20], hw2[dg[0, 0]:dg[0, 0] + 20]) and not np.array_equal(hw[dg[0, 0] + 20:dg[0, 0] + 60], hw2[dg[0, 0] + 20:dg[0, 0] + 60])
    assert sorted(set(roc0.values())) == [0, 1]
    perm = rng.permutation(n)
    keep = np.array([perm[i] for i in range(n) if i % 5 != 4])
    t1, t2 = int(keep[3]), int(keep[11])
    wire[int(dg[t1, 0]) + 30] ^= 0x04
    wire[int(dg[t2, 0] + dg[t2, 1]) - 1] ^= 0x80
    out, ucnt = rtp.unprotect(dev(torch, dg[keep]), wire)
    assert cnt_of(rtp, ucnt) == dict(dict.fromkeys(S.VERDICTS, 0), ok=len(keep) - 2, auth_failed=2)
    rx = ring_handle(N, [FIRST] * N, depth=P)
    arr, lv, sq, pcnt = rtp.parse(rx, out, wire, level=True)
    pc = rtp.parse_count(pcnt)
    assert pc["accepted"] == pc["with_level"] == len(keep) - 2 and pc["malformed"] == 2
    rx.recv_insert(arr, wire)
    assert rx.recv_stats() == dict(inserted=len(keep) - 2, late=0, ahead=0, duplicate=0, bad=2)
    got, st = rx.recv_decode(P)
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


# ---- SRTCP ------------------------------------------------------------------------------------------------------------------------------------------------
def rtcp_session(ses, keys=None, tx_state=None, rx_state=None):
    """test_gpu_srtcp.gpu_session with the GCM entries set through set_rtcp_keys_gcm"""
    r = GC.gpu_session(ses, {s: k for s, k in (keys or {}).items() if not k.get("gcm")}, tx_state, rx_state)
    for d in ("tx", "rx"):
        ss = sorted(k for k, v in (keys or {}).items() if v.get("gcm") and v.get(d) is not None)
        if ss and d == "tx":
            r.set_rtcp_keys_gcm(ss, tx=[keys[k]["tx"] for k in ss], tx_index=[(tx_state or {}).get(k, 0) for k in ss])
        elif ss:
            r.set_rtcp_keys_gcm(ss, rx=[keys[k]["rx"] for k in ss], rx_index=[(rx_state or {}).get(k, -1) for k in ss])
    return r


@pytest.mark.parametrize("n", [1, TILE + 1])
def test_srtcp_build_protect_unprotect_parse(torch_cuda, n):
    """build -> protect_rtcp -> unprotect_rtcp -> parse in a session of both transforms, against the model; the indices advance; the first
    call's datagrams are dropped as replays by a second call; a datagram with E = 0 is accepted"""
    torch = torch_cuda
    N = 8 if n == 1 else n + 3
    rng = np.random.default_rng(2100 + n)
    X, Y = CPUC.sessions(N)
    gcm = [s for s in range(N) if s % 3 != 2]                          # two streams in three under GCM, the third under HMAC
    keys = CPU.rtcp_keys(rng, N, gcm, no_tx=(5,) if n > 1 else ())
    tx_state = {s: int(rng.integers(0, 2 ** 31 - 10)) for s in range(N)}
    if n > 1:
        tx_state.update({0: 0, 1: 65535, 3: 2 ** 31 - 1, 4: 2 ** 31, 5: 0})
    model = CPUC.fill_state(rng, RC.Model(N))
    g = GC.GpuRtcp(torch, N, model.words(), trailer=20)
    tx, rx = rtcp_session(X, keys, tx_state), GC.gpu_session(Y)
    peer_keys = {s: dict(k, tx=None, rx=k["tx"]) for s, k in keys.items()}
    peer, ours = rtcp_session(X, peer_keys), GC.gpu_session(Y)
    streams = [1] if n == 1 else list(range(n))
    rx_state = {s: -1 for s in range(N)}
    first = ok_first = None
    for call in range(2):
        need = CM.model_build_trailer(copy.deepcopy(model), X, Y, streams, GC.NOW + call, 2 ** 40, 20)[3]["bytes_needed"]
        dg, wire, bcnt, idx = g.build(tx, rx, streams, GC.NOW + call, need, need)
        refused, mdg, mwire, mc = CM.model_build_trailer(model, X, Y, streams, GC.NOW + call, need, 20)
        hdg, hwire = host(torch, dg), host(torch, wire)
        assert hdg[:len(streams)].tolist() == [list(d) for d in mdg] and hwire[:len(mwire)].tobytes() == mwire
        want = G.model_protect_rtcp(keys, tx_state, N, streams, False, hdg[:len(streams)], hwire)
        got = GC.protect(torch, g.o, tx, idx, bcnt, dg, wire, int(wire.shape[0]))
        print("srtcp_protect (GCM and HMAC streams) %d reports: %s" % (len(streams), got))
        assert got == want["count"] and sum(got.values()) == len(streams), (got, want["count"])
        hdg, hwire = host(torch, dg), host(torch, wire)
        assert np.array_equal(hdg[:len(streams)], want["dgrams"]) and (hdg[len(streams):] == GC.FILL32).all()
        assert np.array_equal(hwire, want["wire"]) and (hwire[need:] == GC.FILL8).all()
        tx_state = want["tx_state"]
        assert tx.rtcp_index() == ([tx_state[s] for s in range(N)], [-1] * N)
        if n > 1:
            assert got["no_key"] == 1 and got["exhausted"] == 1 + call and got["ok"] == n - 2 - call
        # the receiving end: the bytes moved to another alignment; in the first call a datagram with E = 0 of a stream the build did not
        # list; in the second call the first call's datagrams once more behind the new ones: replays
        shift = 1 + call
        live = hdg[:len(streams)] + np.array([shift, 0], np.int32) * (hdg[:len(streams), 1:] > 0)
        moved = np.concatenate([np.zeros(shift, np.uint8), hwire[:need]])
        if call == 0:
            k0 = G.session_keys(keys[N - 1]["tx"], 3)
            e0 = G.protect_rtcp_packet(k0, RC.write_rr(X.ssrc[N - 1]) + RC.write_sdes(X.ssrc[N - 1], b"e0"), 5, e=0)
            live = np.concatenate([live, np.array([[moved.size, len(e0)]], np.int32)])
            moved = np.concatenate([moved, np.frombuffer(e0, np.uint8)])
            first = (live.copy(), moved.copy())
        else:
            live = np.concatenate([live, first[0] + np.array([moved.size, 0], np.int32) * (first[0][:, 1:] > 0)])
            moved = np.concatenate([moved, first[1]])
        wantu = G.model_unprotect_rtcp(X, peer_keys, rx_state, live, moved)
        d_live, d_moved = dev(torch, live), dev(torch, moved)
        out, uc = GC.unprotect(torch, peer, d_live, d_moved)
        print("srtcp_unprotect (GCM and HMAC streams) %d datagrams: %s" % (live.shape[0], uc))
        assert uc == wantu["count"] and sum(uc.values()) == live.shape[0], (uc, wantu["count"])
        m = live.shape[0]
        assert np.array_equal(host(torch, out)[:m], wantu["dgrams"]) and np.array_equal(host(torch, d_moved), wantu["wire"])
        if call == 0:
            assert wantu["verdicts"][-1] == "ok" and uc["ok"] == got["ok"] + 1 and keys[N - 1].get("gcm")
            ok_first = uc["ok"]
        else:
            assert uc["replayed"] == ok_first and uc["ok"] == got["ok"]
        rx_state = wantu["rx_state"]
        assert peer.rtcp_index()[1] == [rx_state[s] for s in range(N)]
        fb, pcnt = GC.GpuRtcp(torch, N).o.parse(peer, ours, out[:m].contiguous(), d_moved, GC.NOW + 5)
        assert int(host(torch, pcnt)[0]) == uc["ok"]
    # the trailer switch: 20 is accepted, 17 .. 19 and 21 are not; below 20 the call is refused while the session holds a GCM tx key
    assert g.lib.solo_rtcp_set_trailer(g.h, 19) == -1 and g.lib.solo_rtcp_set_trailer(g.h, 21) == -1 and g.lib.solo_rtcp_set_trailer(g.h, 16) == 0
    cnt = torch.full((8,), -9, dtype=torch.int32, device="cuda")
    keep = host(torch, wire).copy()
    assert tx.lib.solo_srtcp_protect(g.h, tx.h, idx.data_ptr(), len(streams), bcnt.data_ptr(), dg.data_ptr(), wire.data_ptr(), int(wire.shape[0]), cnt.data_ptr(), tx._stream()) == -1
    g.o.trailer = 16                                                  # (the binding's view of the switch, as the library's stands)
    with pytest.raises(ValueError, match="20"):                        # the library's -1 under a trailer below 20: the binding says what it means
        tx.protect_rtcp(g.o, idx, bcnt[:8], dg[:len(streams)], wire)
    assert (host(torch, cnt) == -9).all() and np.array_equal(host(torch, wire), keep)
    tx.clear_rtcp_keys(gcm)                                           # no GCM tx key is left: 14 is enough again
    g.o.set_trailer(14)
    assert GC.protect(torch, g.o, tx, idx, bcnt, dg, wire, int(wire.shape[0]))["ok"] >= 0


# ---- capture ----------------------------------------------------------------------------------------------------------------------------------------------
def test_capture_srtp_gcm_protect_and_unprotect(torch_cuda):
    """solo_send_pack, solo_rtp_pack, solo_srtp_protect and -- on the receiving session, over a copy the graph makes -- solo_srtp_unprotect
    in one graph, the sessions keyed for GCM (streams 6 and 7 for AES-CM): replays with other packets of the fixture equal the same calls
    made eagerly on a twin, and the model"""
    import solo_amd
    torch = torch_cuda
    z = GR.fixture()
    P, SLOT, MAXR, WCAP = 3, z["bits"].shape[2], 48, 16384
    rng = np.random.default_rng(198)
    ses = R.random_session(rng, 8, 640, 3)
    ses["srtp"] = {s: G.gcm_entry(rng) if s < 6 else CPU.cm_entry(rng, 10) for s in range(8)}
    for k in ses["srtp"].values():
        k["rx"] = k["tx"]
    roc0 = {s: (ses["streams"][s]["seq_offset"] + 1000) >> 16 for s in range(8)}

    def make():
        h = solo_amd.SoloBatch(8, encoder=False, decoder=True, slot_bytes=SLOT)
        rtp, peer = srtp_session(ses), srtp_session(ses, roc0)
        ins = dict(bits=GR.zeros(torch, (8, P, SLOT), torch.uint8), nbytes=GR.zeros(torch, (8, P, 2), torch.int16), level=GR.zeros(torch, (8, 4), torch.uint8))
        outs = dict(records=GR.zeros(torch, (MAXR, 5), torch.int32), payload=GR.zeros(torch, (8 * P * SLOT,), torch.uint8), scount=GR.zeros(torch, (8,), torch.int32),
                    dgrams=GR.zeros(torch, (MAXR, 2), torch.int32), wire=GR.zeros(torch, (WCAP,), torch.uint8), count=GR.zeros(torch, (8,), torch.int32),
                    scnt=GR.zeros(torch, (8,), torch.int32), work=GR.zeros(torch, (WCAP,), torch.uint8), back=GR.zeros(torch, (MAXR, 2), torch.int32),
                    ucnt=GR.zeros(torch, (8,), torch.int32))

        def call():
            r = h.lib.solo_send_pack(h.h, ins["bits"].data_ptr(), ins["nbytes"].data_ptr(), None, P, None, 500, outs["records"].data_ptr(), MAXR,
                                     outs["payload"].data_ptr(), 8 * P * SLOT, outs["scount"].data_ptr(), h._stream())
            r = r or rtp.lib.solo_rtp_pack(rtp.h, outs["records"].data_ptr(), outs["scount"].data_ptr(), MAXR, outs["payload"].data_ptr(), 8 * P * SLOT,
                                           ins["level"].data_ptr(), 4, outs["dgrams"].data_ptr(), outs["wire"].data_ptr(), WCAP, outs["count"].data_ptr(), rtp._stream())
            r = r or rtp.lib.solo_srtp_protect(rtp.h, outs["records"].data_ptr(), outs["scount"].data_ptr(), MAXR, outs["dgrams"].data_ptr(), outs["wire"].data_ptr(),
                                               WCAP, outs["scnt"].data_ptr(), rtp._stream())
            outs["work"].copy_(outs["wire"])
            return r or peer.lib.solo_srtp_unprotect(peer.h, outs["dgrams"].data_ptr(), MAXR, outs["work"].data_ptr(), WCAP, outs["back"].data_ptr(), outs["ucnt"].data_ptr(),
                                                     peer._stream())
        return GR.Stage(torch, ins, outs, call, keep=(h, rtp, peer))

    feeds = [dict(bits=z["bits"][:, 3 * k:3 * k + 3], nbytes=z["nbytes"][:, 3 * k:3 * k + 3], level=rng.integers(0, 255, (8, 4), dtype=np.uint8)) for k in range(4)]

    def model(k, feed, got):
        n = int(got["scount"][0])
        wp = S.model_pack_trailer(R, ses, got["records"], n, got["payload"], feed["level"], 16, MAXR, WCAP)
        want = G.model_protect(ses, got["records"], n, wp["dgrams"], np.concatenate([wp["wire"], np.zeros(64, np.uint8)]), MAXR)
        assert 0 < n <= MAXR and got["scnt"].tolist() == [n, 0, 0, 0, 0, 0, 0, 0], (k, n, got["scnt"])
        nb = wp["count"]["bytes"]
        assert np.array_equal(got["dgrams"][:n], want["dgrams"][:n]) and np.array_equal(got["wire"][:nb], want["wire"][:nb])
        assert (got["wire"][nb:] == GR.FILL).all() and (got["dgrams"][n:].view(np.uint8) == GR.FILL).all()
        assert got["ucnt"].tolist()[:3] == [n, 0, MAXR - n] and np.array_equal(got["back"][:n, 0], wp["dgrams"][:n, 0]) and np.array_equal(got["back"][:n, 1], wp["dgrams"][:n, 1])
        for off, ln in got["back"][:n].tolist():
            assert np.array_equal(got["work"][off:off + ln], wp["wire"][off:off + ln])

    GR.replay_against_twin(torch, make, feeds, model=model)


def test_capture_srtcp_gcm_protect_and_unprotect(torch_cuda):
    """solo_rtcp_build with the 20-byte trailer, solo_srtcp_protect and -- on the peer's session, over a copy the graph makes --
    solo_srtcp_unprotect in one graph, two streams in three under GCM: every replay stamps another time and ADVANCES THE INDICES of both
    ends, so its bytes differ from the replay before and equal the model's"""
    torch = torch_cuda
    n, CAP = 70, 120 * 70
    rng = np.random.default_rng(2500)
    X, Y = CPUC.sessions(n)
    keys = CPU.rtcp_keys(rng, n, [s for s in range(n) if s % 3 != 2], no_tx=(5,))
    peer_keys = {s: dict(k, tx=None, rx=k["tx"]) for s, k in keys.items()}
    start = {s: int(rng.integers(0, 70000)) for s in range(n)}
    model = CPUC.fill_state(rng, RC.Model(n))
    w0 = model.words().copy()
    ry = GC.gpu_session(Y)
    streams = list(range(1, n))

    def make():
        a, tx, peer = GC.GpuRtcp(torch, n, w0, trailer=20), rtcp_session(X, keys, start), rtcp_session(X, peer_keys)
        ins = dict(now=GR.zeros(torch, (1,), torch.int64))
        outs = dict(dgrams=GR.zeros(torch, (n - 1, 2), torch.int32), wire=GR.zeros(torch, (CAP,), torch.uint8), bcount=GR.zeros(torch, (8,), torch.int32),
                    count=GR.zeros(torch, (8,), torch.int32), work=GR.zeros(torch, (CAP,), torch.uint8), back=GR.zeros(torch, (n - 1, 2), torch.int32),
                    ucount=GR.zeros(torch, (8,), torch.int32))
        idx = dev(torch, np.array(streams, np.int32))

        def call():
            r = a.lib.solo_rtcp_build(a.h, tx.h, ry.h, idx.data_ptr(), n - 1, 1, ins["now"].data_ptr(), outs["dgrams"].data_ptr(), outs["wire"].data_ptr(), CAP,
                                      outs["bcount"].data_ptr(), a.o._stream())
            r = r or tx.lib.solo_srtcp_protect(a.h, tx.h, idx.data_ptr(), n - 1, outs["bcount"].data_ptr(), outs["dgrams"].data_ptr(), outs["wire"].data_ptr(), CAP,
                                               outs["count"].data_ptr(), tx._stream())
            outs["work"].copy_(outs["wire"])
            return r or peer.lib.solo_srtcp_unprotect(peer.h, outs["dgrams"].data_ptr(), n - 1, outs["work"].data_ptr(), CAP, outs["back"].data_ptr(),
                                                      outs["ucount"].data_ptr(), peer._stream())

        def state():
            return np.concatenate([a.words().ravel().astype(np.int64), np.array(tx.rtcp_index()[0], np.int64), np.array(peer.rtcp_index()[1], np.int64)])
        return GR.Stage(torch, ins, outs, call, state=state, keep=(a, tx, peer, idx))

    feeds = [dict(now=np.array([(0x83AA7E80 + 5 * k << 32) | (k << 20)], np.uint64).view(np.int64)) for k in range(3)]
    st = dict(tx=dict(start), rx={s: -1 for s in range(n)})

    def check(k, feed, got):
        now = int(feed["now"].view(np.uint64)[0])
        _, md, mw, mc = CM.model_build_trailer(model, X, Y, streams, now, CAP, 20)
        plain = np.full(CAP, GR.FILL, np.uint8)
        plain[:len(mw)] = np.frombuffer(mw, np.uint8)
        want = G.model_protect_rtcp(keys, st["tx"], n, streams, False, md, plain)
        assert CPUC.build_count_of(got["bcount"]) == mc and GC.count_dict(got["count"]) == want["count"] == dict(ZERO, ok=n - 2, no_key=1)
        assert np.array_equal(got["dgrams"], want["dgrams"]) and np.array_equal(got["wire"], want["wire"])
        st["tx"] = want["tx_state"]
        wu = G.model_unprotect_rtcp(X, peer_keys, st["rx"], want["dgrams"], want["wire"])
        assert GC.count_dict(got["ucount"]) == wu["count"] == dict(ZERO, ok=n - 2, malformed=1) and np.array_equal(got["back"], wu["dgrams"])
        assert np.array_equal(got["work"], wu["wire"])
        st["rx"] = wu["rx_state"]

    _, cap, twin = GR.replay_against_twin(torch, make, feeds, model=check, stateful=True)
    index = cap.keep[1].rtcp_index()[0]
    assert all(index[s] == st["tx"][s] == start[s] + 3 for s in streams if s != 5) and cap.keep[2].rtcp_index()[1] == [st["rx"][s] for s in range(n)]

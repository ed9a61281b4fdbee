"""The SRTP stage (solo_srtp_protect / solo_srtp_unprotect, solo_amd/csrc/solo_srtp.h) without a GPU: the per-datagram functions, the host
forms and the control plane are compiled for the host by this test (tests/srtp_host.cpp, through tests/host_build.py) and compared byte
for byte with the independent model of tests/srtp_model.py, whose pieces are pinned by published answers (FIPS-197 C.1, RFC 3711 B.2 and
B.3, RFC 2202 case 1).  Then pack's trailer, the control plane's refusals, the ABI, the built library's new kernels (no scratch), and the
hostile family once more through a stand-alone build of the same source under the address and undefined-behaviour sanitisers."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import solo_testlib as T
import rtp_model as R
import srtp_model as M
from host_build import FLAGS, host_lib, source

SRTP_SYMBOLS = ("solo_rtp_set_trailer", "solo_srtp_set_keys", "solo_srtp_clear_keys", "solo_srtp_get_rx_index", "solo_srtp_protect", "solo_srtp_unprotect")
KERNELS = ("solo_srtp_protect_kernel", "solo_srtp_unprotect_kernel", "solo_srtp_rx_fold_kernel")
FILL = 0xA5
H = bytes.fromhex


@pytest.fixture(scope="module")
def host():
    lib = host_lib("srtp")
    V, I, LL = C.c_void_p, C.c_int, C.c_longlong
    lib.emu_srtp_create.restype = V
    lib.emu_srtp_create.argtypes = [I, I]
    lib.emu_srtp_destroy.argtypes = [V]
    lib.emu_srtp_bind.argtypes = [V, V, I] + [V] * 5 + [I]
    lib.emu_srtp_unbind.argtypes = [V, V, I]
    lib.emu_srtp_set_trailer.argtypes = [V, I]
    lib.emu_srtp_set_keys.argtypes = [V, V, I, V, V, V, I]
    lib.emu_srtp_clear_keys.argtypes = [V, V, I]
    lib.emu_srtp_rx_index.argtypes = [V, V, I, V]
    lib.emu_srtp_mirror.argtypes = [V, I, I]
    lib.emu_srtp_key_words.argtypes = [V, I]
    lib.emu_srtp_pack.argtypes = [V, V, V, I, V, LL, V, I, V, V, LL, V]
    lib.emu_srtp_protect.argtypes = [V, V, V, I, V, V, LL, V]
    lib.emu_srtp_unprotect.argtypes = [V, V, I, V, LL, V, V]
    lib.emu_aes_block.argtypes = [V, V, V]
    lib.emu_aes_cm.argtypes = [V, V, C.c_uint, V]
    lib.emu_srtp_derive.argtypes = [V] * 5
    lib.emu_hmac.argtypes = [V, I, V, I, C.c_uint, I, V]
    lib.emu_srtp_guess.restype = LL
    lib.emu_srtp_guess.argtypes = [LL, C.c_uint, C.c_uint]
    return lib


def p(x):
    return None if x is None else x.ctypes.data


def count_dict(cnt):
    return dict(zip(M.VERDICTS + ("reserved0", "reserved1"), (int(v) for v in cnt)))


class HostSrtp:
    """the host form's session: bound and keyed as the model's session dict says"""

    def __init__(self, lib, ses, trailer=None, roc0=None):
        self.lib, self.ses = lib, ses
        self.h = lib.emu_srtp_create(ses["n_streams"], ses["L"])
        s = sorted(ses["streams"])
        c = [ses["streams"][k] for k in s]
        a = [np.array(s, np.int32), np.array([x["ssrc"] for x in c], np.uint32), np.array([x["ts_offset"] for x in c], np.uint32),
             np.array([x["seq_offset"] for x in c], np.uint16), np.array([x["pt"][0] for x in c], np.uint8), np.array([x["pt"][1] for x in c], np.uint8)]
        assert lib.emu_srtp_bind(self.h, p(a[0]), len(s), p(a[1]), p(a[2]), p(a[3]), p(a[4]), p(a[5]), ses["level_id"]) == 0
        tags = {k["tag"] for k in ses.get("srtp", {}).values()}
        if trailer is None:
            trailer = max(tags) if tags else 0
        assert self.set_trailer(trailer) == 0
        for tag in sorted(tags):
            for d in ("tx", "rx"):
                ss = [s for s, k in sorted(ses["srtp"].items()) if k["tag"] == tag and k.get(d) is not None]
                if ss:
                    roc = None if d == "tx" or roc0 is None else [roc0.get(s, 0) for s in ss]
                    assert self.set_keys(ss, tag, **{d: [ses["srtp"][s][d] for s in ss]}, roc=roc) == 0

    def set_trailer(self, t):
        return self.lib.emu_srtp_set_trailer(self.h, t)

    def set_keys(self, streams, tag, tx=None, rx=None, roc=None):
        s = np.array(streams, np.int32)
        txa = None if tx is None else np.frombuffer(b"".join(tx), np.uint8)
        rxa = None if rx is None else np.frombuffer(b"".join(rx), np.uint8)
        ra = None if roc is None else np.array(roc, np.uint32)
        return self.lib.emu_srtp_set_keys(self.h, p(s), len(streams), p(txa), p(rxa), p(ra), tag)

    def clear_keys(self, streams):
        s = np.array(streams, np.int32)
        return self.lib.emu_srtp_clear_keys(self.h, p(s), len(streams))

    def unbind(self, streams):
        s = np.array(streams, np.int32)
        return self.lib.emu_srtp_unbind(self.h, p(s), len(streams))

    def rx_index(self, streams=None):
        s = np.array(range(self.ses["n_streams"]) if streams is None else streams, np.int32)
        out = np.full(s.size, -5, np.int64)
        assert self.lib.emu_srtp_rx_index(self.h, p(s), s.size, p(out)) == 0
        return out.tolist()

    def pack(self, records, n_records, payload, level=None, cap=None, guard=64):
        """-> (dgrams [max,2], wire [cap + guard] in a buffer with FILL around it, count dict)"""
        records = np.ascontiguousarray(records, np.int32)
        m = records.shape[0]
        cap = 4 * (int(payload.size) + 40 * m) if cap is None else cap
        sc = np.zeros(8, np.int32)
        sc[0] = n_records
        dg = np.full((m, 2), -7, np.int32)
        backing = np.full(cap + guard + 16, FILL, np.uint8)
        a0 = (-backing.ctypes.data) % 4 + 4
        wire = backing[a0:a0 + cap + guard]
        cnt = np.full(8, -9, np.int32)
        self.lib.emu_srtp_pack(self.h, p(records), p(sc), m, p(payload), payload.size, p(level), 0 if level is None else level.shape[1], p(dg), p(wire), cap, p(cnt))
        c = dict(dgrams=int(cnt[0]), dgrams_needed=int(cnt[1]), bytes=int(cnt[2:4].view(np.int64)[0]), bytes_needed=int(cnt[4:6].view(np.int64)[0]),
                 refused=int(cnt[6]), reserved=int(cnt[7]))
        assert (wire[cap:] == FILL).all() and (backing[:a0] == FILL).all()
        return dg, wire, c

    def protect(self, records, n_records, dg, wire, wire_bytes=None, max_records=None):
        records = np.ascontiguousarray(records, np.int32)
        sc = np.zeros(8, np.int32)
        sc[0] = n_records
        cnt = np.full(8, -9, np.int32)
        self.lib.emu_srtp_protect(self.h, p(records), p(sc), records.shape[0] if max_records is None else max_records, p(dg), p(wire),
                                  wire.size if wire_bytes is None else wire_bytes, p(cnt))
        return count_dict(cnt)

    def unprotect(self, dg, wire, wire_bytes=None):
        dg = np.ascontiguousarray(dg, np.int32).reshape(-1, 2)
        out = np.full((dg.shape[0] + 4, 2), -7, np.int32)
        cnt = np.full(8, -9, np.int32)
        self.lib.emu_srtp_unprotect(self.h, p(dg), dg.shape[0], p(wire), wire.size if wire_bytes is None else wire_bytes, p(out), p(cnt))
        assert (out[dg.shape[0]:] == -7).all()
        return out[:dg.shape[0]], count_dict(cnt)

    def close(self):
        self.lib.emu_srtp_destroy(self.h)


def lay_out(rng, dgs, front=0, gap=3, align=None):
    """datagrams (bytes) -> (dgrams int32 [n,2], wire uint8 with FILL between): at every byte alignment, or all at `align` mod 4"""
    wire, table = bytearray([FILL] * front), []
    for d in dgs:
        wire += bytes([FILL]) * int(rng.integers(0, gap + 1))
        if align is not None:
            wire += bytes([FILL]) * ((align - len(wire)) % 4)
        table.append((len(wire), len(d)))
        wire += d
    wire += bytes([FILL]) * 8
    return np.array(table, np.int32).reshape(-1, 2), np.frombuffer(bytes(wire), np.uint8).copy()


# ---- published answers: through the model, then through the host form's pieces -------------------------------------------------------------------
B2_KEY, B2_IV = H("2B7E151628AED2A6ABF7158809CF4F3C"), H("F0F1F2F3F4F5F6F7F8F9FAFBFCFD0000")
B2 = {0: "E03EAD0935C95E80E166B16DD92B4EB4", 1: "D23513162B02D0F72A43A2FE4A5F97AB", 2: "41E95B3BB0A2E8DD477901E4FCA894C0",
      0xFEFF: "EC8CDF7398607CB0F2D21675EA9EA1E4", 0xFF00: "362B7C3C6773516318A077D7FC5073AE", 0xFF01: "6A2CC3787889374FBEB4C81B17BA6C44"}
B3_MASTER = H("E1F97A0D3E018BE0D64FA32C06DE4139") + H("0EC675AD498AFEEBB6960B3AABE6")
B3 = dict(ke=H("C61E7A93744F39EE10734AFE3FF7A087"), ks=H("30CBBC08863D8C85D49DB34A9AE1"), ka=H("CEBE321F6FF7716B6FD4AB49AF256A156D38BAA4"))


def test_model_known_answers():
    assert M.aes_encrypt(bytes(range(16)), H("00112233445566778899aabbccddeeff")) == H("69c4e0d86a7b0430d8cdb78070b4c55a")
    for j, want in B2.items():
        assert M.aes_cm(B2_KEY, int.from_bytes(B2_IV, "big"), 16, first_block=j) == H(want), j
    assert M.session_keys(B3_MASTER) == B3
    import hashlib
    import hmac
    assert hmac.new(b"\x0b" * 20, b"Hi There", hashlib.sha1).digest() == H("b617318655057264e28bc0b6fb378c8ef146be00")


def test_host_known_answers(host):
    def buf(b):
        return np.frombuffer(bytes(b), np.uint8).copy()
    out = np.zeros(16, np.uint8)
    key, block = buf(range(16)), buf(H("00112233445566778899aabbccddeeff"))          # (named: an array lives as long as its name)
    host.emu_aes_block(p(key), p(block), p(out))
    assert out.tobytes() == H("69c4e0d86a7b0430d8cdb78070b4c55a")
    key, iv = buf(B2_KEY), buf(B2_IV)
    for j, want in B2.items():
        host.emu_aes_cm(p(key), p(iv), j, p(out))
        assert out.tobytes() == H(want), j
    ke, ks, ka, rec, master = np.zeros(16, np.uint8), np.zeros(14, np.uint8), np.zeros(20, np.uint8), np.zeros(64, np.uint32), buf(B3_MASTER)
    host.emu_srtp_derive(p(master), p(ke), p(ks), p(ka), p(rec))
    assert dict(ke=ke.tobytes(), ks=ks.tobytes(), ka=ka.tobytes()) == B3
    # the record: round keys of k_e (the first four are the key itself), the salt shifted to its place, tag length, "has key"
    assert rec[:4].astype(">u4").tobytes() == B3["ke"] and rec[44:48].astype(">u4").tobytes() == B3["ks"] + b"\x00\x00"
    assert rec[58] == 10 and rec[59] == 1 and not rec[60:].any()
    assert host.emu_srtp_sizes(0) == 32 and host.emu_srtp_sizes(1) == 256 and host.emu_srtp_sizes(2) == 32 and host.emu_srtp_sizes(3) == 32
    # HMAC from the midstates: RFC 2202 case 1, then random messages of every length around the padding edges at every alignment
    mac = np.zeros(20, np.uint8)
    key, msg = buf(b"\x0b" * 20), buf(b"Hi There")
    host.emu_hmac(p(key), 20, p(msg), 8, 0, 0, p(mac))
    assert mac.tobytes() == H("b617318655057264e28bc0b6fb378c8ef146be00")
    import hashlib
    import hmac
    rng = np.random.default_rng(1)
    for n in list(range(0, 70)) + [118, 119, 120, 121, 127, 128, 129, 300]:
        for al in range(4):
            key, backing = rng.integers(0, 256, 20, dtype=np.uint8), rng.integers(0, 256, n + 8, dtype=np.uint8)
            a0 = (al - backing.ctypes.data) % 4
            msg = backing[a0:a0 + n]
            host.emu_hmac(p(key), 20, p(msg), n, 0x01020304, 4, p(mac))
            assert mac.tobytes() == hmac.new(key.tobytes(), msg.tobytes() + b"\x01\x02\x03\x04", hashlib.sha1).digest(), (n, al)


def test_aes_table_is_the_column_of_the_sbox():
    text = open(os.path.join(T.ROOT, "solo_amd", "csrc", "solo_srtp_tables.inc")).read()
    te = [int(w.rstrip("u"), 16) for w in text.replace(",", " ").split() if w.startswith("0x")]
    assert len(te) == 256
    for x, s in enumerate(M.SBOX):
        assert te[x] == (M._gmul(s, 2) << 24) | (s << 16) | (s << 8) | M._gmul(s, 3), x


# ---- protect -------------------------------------------------------------------------------------------------------------------------------------------
def protect_case(rng, with_level, tag):
    """a session of 6 streams and records over them: every edge length; sender indices around the 16-bit wrap (seq_offset 65534 with
    packets 0 and 1: ROC 0 and 1 inside one packet's two descriptions) and at the mod-2^32 edge (65535 with seq 2^31 - 1); stream 4
    without a tx key; stream 5 not bound"""
    Hb = 20 if with_level else 12
    ses = R.random_session(rng, 6, 640, 3, unbound=(5,))
    ses["streams"][0]["seq_offset"], ses["streams"][1]["seq_offset"] = 65534, 65535
    ses["streams"][2]["seq_offset"], ses["streams"][3]["seq_offset"] = 1000, 40000
    M.random_keys(rng, ses, tag, no_tx=(4,))
    lens = M.edge_lengths(Hb)
    rec, at = [], 0
    for i, ln in enumerate(lens):
        rec.append([2 + i % 2, 100 + i, i % 2, at, ln])
        at += ln - 1                                                  # (ranges overlap: the pool is read, never written)
    rec += [[0, 0, 0, 3, 40], [0, 0, 1, 5, 41], [0, 1, 0, 7, 42], [0, 1, 1, 9, 43], [1, 2 ** 31 - 1, 0, 11, 44], [1, 2 ** 31 - 1, 1, 13, 45], [1, 32767, 1, 2, 46],
            [4, 7, 0, 0, 30], [5, 7, 0, 0, 30], [2, 8, 2, 0, 30]]
    rec = np.array(rec, np.int32)
    pool = rng.integers(0, 256, at + 300, dtype=np.uint8)
    level = rng.integers(0, 255, (6, 4), dtype=np.uint8) if with_level else None
    return ses, rec, pool, level


@pytest.mark.parametrize("tag", [10, 4])
@pytest.mark.parametrize("with_level", [False, True])
def test_host_protect_against_model(host, with_level, tag):
    rng = np.random.default_rng(40 + tag + with_level)
    ses, rec, pool, level = protect_case(rng, with_level, tag)
    h = HostSrtp(host, ses)
    n = rec.shape[0]
    dg, wire, c = h.pack(rec, n, pool, level)
    want_pack = M.model_pack_trailer(R, ses, rec, n, pool, level, tag)
    assert c == want_pack["count"] and c["refused"] == 2 and np.array_equal(dg, want_pack["dgrams"]) and np.array_equal(wire[:c["bytes"]], want_pack["wire"])
    packed_dg, packed = dg.copy(), wire.copy()
    want = M.model_protect(ses, rec, n, dg, wire)
    got = h.protect(rec, n, dg, wire)
    assert got == want["count"] and got == dict(want["count"], ok=n - 3, skipped=2, no_key=1, malformed=0, unknown_ssrc=0, auth_failed=0)
    assert np.array_equal(dg, want["dgrams"]) and np.array_equal(wire, want["wire"])
    live = dg[:, 1] > 0
    assert (dg[live, 1] == packed_dg[live, 1] + tag).all() and tuple(dg[n - 3]) == (0, 0) and tuple(packed_dg[n - 3]) != (0, 0)
    # the rollover counters of the wrap records: 0, 0 | 1, 1 ... and 2^32 mod 2^32 at the far end
    Hb = 20 if with_level else 12
    for k, roc in ((12, 0), (13, 0), (14, 1), (15, 1), (16, 65536), (17, 65536), (18, 1)):
        off, ln = packed_dg[k]
        stream = int(rec[k, 0])
        sp = M.protect_packet(M.session_keys(ses["srtp"][stream]["tx"]), tag, packed[off:off + ln].tobytes(), roc)
        assert wire[off:off + ln + tag].tobytes() == sp, k
    # header (and the level in it) stays readable, the payload does not
    for k in np.nonzero(live)[0]:
        off = dg[k, 0]
        assert np.array_equal(wire[off:off + Hb], packed[off:off + Hb])
    assert not np.array_equal(wire[dg[5, 0] + Hb:dg[5, 0] + Hb + 200], packed[dg[5, 0] + Hb:dg[5, 0] + Hb + 200])
    # loopback: the receiving end's unprotect gives back the packed bytes, tag bytes aside
    rx = HostSrtp(host, M.loop_session(ses), roc0={0: 0, 1: 65536})
    # (streams 0 and 1 carry two rollover counters in one call, more than 2^15 apart or not: fed per counter below)
    for sel in (np.nonzero(live & (rec[:, 0] >= 2))[0], [12, 13], [14, 15], [16], ):
        sub = dg[list(sel)]
        w2 = wire.copy()
        out, cu = rx.unprotect(sub, w2)
        assert cu["ok"] == len(sub), (sel, cu)
        assert np.array_equal(out[:, 0], sub[:, 0]) and np.array_equal(out[:, 1], sub[:, 1] - tag)
        for (off, ln) in out:
            assert np.array_equal(w2[off:off + ln], packed[off:off + ln])
    # a refused list; a cut by max_records; a tag that would reach past wire_bytes
    dg2, w2 = packed_dg.copy(), packed.copy()
    assert h.protect(rec, -1, dg2, w2) == dict(want["count"], ok=-1, skipped=0, no_key=0) and np.array_equal(dg2, packed_dg) and np.array_equal(w2, packed)
    assert h.protect(rec, n, dg2, w2, max_records=5)["ok"] == 5 and np.array_equal(dg2[5:], packed_dg[5:]) and np.array_equal(dg2[:5], dg[:5])
    dg2, w2 = packed_dg.copy(), packed.copy()
    last = int(np.nonzero(live)[0][-1])
    end = int(packed_dg[last].sum())
    for wb, ok in ((end + tag, True), (end + tag - 1, False), (end - 1, False)):
        dg3, w3 = packed_dg.copy(), packed.copy()
        cm = M.model_protect(ses, rec, n, dg3.copy(), w3, wire_bytes=wb)
        got = h.protect(rec, n, dg3, w3, wire_bytes=wb)
        assert got == cm["count"] and np.array_equal(dg3, cm["dgrams"]) and np.array_equal(w3, cm["wire"])
        assert (tuple(dg3[last]) != (0, 0)) == ok and got["malformed"] >= (0 if ok else 1)
    h.close()
    rx.close()


def test_fanout_three_streams_one_pool_range(host):
    """one pool range under three streams' keys: three different ciphertexts, each back to the same bytes"""
    rng = np.random.default_rng(8)
    ses = M.random_keys(rng, R.random_session(rng, 3, 640, 0))
    h, rx = HostSrtp(host, ses), HostSrtp(host, M.loop_session(ses))
    pool = rng.integers(0, 256, 100, dtype=np.uint8)
    rec = np.array([[s, 50, 0, 10, 77] for s in range(3)], np.int32)
    dg, wire, c = h.pack(rec, 3, pool)
    want = M.model_protect(ses, rec, 3, dg, wire)
    assert h.protect(rec, 3, dg, wire)["ok"] == 3 and np.array_equal(wire, want["wire"]) and np.array_equal(dg, want["dgrams"])
    body = [wire[o + 12:o + 12 + 77].tobytes() for o in dg[:, 0]]
    assert len(set(body)) == 3 and pool[10:87].tobytes() not in body
    out, cu = rx.unprotect(dg, wire)
    assert cu["ok"] == 3 and all(wire[o + 12:o + 12 + 77].tobytes() == pool[10:87].tobytes() for o in out[:, 0])
    h.close()
    rx.close()


# ---- unprotect: the hostile family ------------------------------------------------------------------------------------------------------------------
def hostile_case(rng, tag, align=None):
    ses = R.random_session(rng, 6, 640, 5, unbound=(3,))
    M.random_keys(rng, ses, tag, no_rx=(4,))
    state = M.new_state(ses, {2: 7})
    kinds = M.hostile_set(ses, state, 2, rng, R) + M.hostile_set(ses, state, 0, rng, R)
    c4 = ses["streams"][4]
    kinds.append(("no_key", R.build(c4["ssrc"], 96, 3, 0, b"x" * 30), "no_key"))
    order = rng.permutation(len(kinds))
    dg, wire = lay_out(rng, [kinds[i][1] for i in order], front=int(rng.integers(0, 4)), align=align)
    return ses, state, [kinds[i] for i in order], dg, wire


@pytest.mark.parametrize("tag", [10, 4])
def test_unprotect_verdicts_in_rule_order(host, tag):
    for align in (0, 1, 2, 3, None):
        rng = np.random.default_rng(70 + tag + (9 if align is None else align))
        ses, state, kinds, dg, wire = hostile_case(rng, tag, align)
        if align is not None:
            assert (dg[:, 0] % 4 == align).all()
        want = M.model_unprotect(ses, state, dg, wire)
        assert want["verdicts"] == [k[2] for k in kinds], [(k[0], k[2], v) for k, v in zip(kinds, want["verdicts"]) if k[2] != v]
        assert set(want["verdicts"]) == {"ok", "malformed", "unknown_ssrc", "no_key", "auth_failed"}
        h = HostSrtp(host, ses, roc0={2: 7})
        before = wire.copy()
        backing = np.full(wire.size + 64, 0x3C, np.uint8)              # guard bytes around the wire
        a0 = 32 + (0 - backing.ctypes.data - 32) % 4
        w = backing[a0:a0 + wire.size]
        w[:] = wire
        out, cnt = h.unprotect(dg, w)
        assert cnt == want["count"], (cnt, want["count"])
        assert np.array_equal(out, want["dgrams"]) and np.array_equal(w, want["wire"])
        assert (backing[:a0] == 0x3C).all() and (backing[a0 + wire.size:] == 0x3C).all()
        # a rejected datagram: every byte as it was; between the datagrams too
        touched = np.zeros(wire.size, bool)
        for (off, ln), v in zip(out, want["verdicts"]):
            if v == "ok":
                touched[off:off + ln] = True
        assert np.array_equal(w[~touched], before[~touched]) and not np.array_equal(w[touched], before[touched])
        assert h.rx_index() == [want["state"][s]["index"] for s in range(6)] and h.rx_index([2])[0] >> 16 == 7
        # ranges that leave the wire are malformed and never read
        bad = np.array([[-1, 40], [wire.size - 39, 40], [wire.size, 16], [2 ** 31 - 1, 2 ** 31 - 1], [0, -5], [0, 0]], np.int32)
        out, cnt = h.unprotect(bad, w)
        assert cnt["malformed"] == 6 and not out.any() and np.array_equal(w, want["wire"])
        h.close()


def test_no_keys_at_all(host):
    """a session that never saw set_keys: unprotect finds no key, protect voids what it is given"""
    rng = np.random.default_rng(3)
    ses = R.random_session(rng, 2, 640, 0)
    ses["srtp"] = {}
    h = HostSrtp(host, ses)
    pool = rng.integers(0, 256, 64, dtype=np.uint8)
    rec = np.array([[0, 1, 0, 0, 20], [1, 1, 1, 20, 20]], np.int32)
    dg, wire, c = h.pack(rec, 2, pool)
    before = wire.copy()
    out, cnt = h.unprotect(dg, wire)
    assert cnt["no_key"] == 2 and not out.any() and np.array_equal(wire, before) and h.rx_index() == [-1, -1]
    assert h.protect(rec, 2, dg, wire)["no_key"] == 2 and not dg.any() and np.array_equal(wire, before)
    h.close()


# ---- the receive index -------------------------------------------------------------------------------------------------------------------------------
def test_receive_index_rule(host):
    for roc in (0, 1, 5, 2 ** 32 - 1):
        for s_l in (0, 1, 100, 32767, 32768, 32769, 65534, 65535):
            for seq in (0, 1, 99, 100, 101, 32767, 32768, 32769, 65534, 65535, (s_l + 32768) % 65536, (s_l + 32767) % 65536, (s_l + 32769) % 65536):
                st = dict(index=(roc << 16) | s_l, roc0=9)
                assert host.emu_srtp_guess(st["index"], 9, seq) == M.guess_index(st, seq), (roc, s_l, seq)
    assert host.emu_srtp_guess(-1, 9, 5) == M.guess_index(dict(index=-1, roc0=9), 5) == (9 << 16) | 5
    # both directions across 65535 / 0
    assert M.guess_index(dict(index=(3 << 16) | 65535, roc0=0), 0) == (4 << 16) | 0
    assert M.guess_index(dict(index=(4 << 16) | 2, roc0=0), 65534) == (3 << 16) | 65534          # a late packet from before the wrap


def stream_of_packets(rng, ses, stream, indices):
    c, k = ses["streams"][stream], ses["srtp"][stream]
    keys = M.session_keys(k["rx"])
    return [M.protect_packet(keys, k["tag"], R.build(c["ssrc"], c["pt"][0], i & 0xFFFF, 0, rng.integers(0, 256, 24, dtype=np.uint8).tobytes()), i >> 16) for i in indices]


def test_receive_index_across_the_wrap(host):
    """call after call across 65535 / 0, with a late packet from before the wrap in a later call and one from after it in an earlier one"""
    rng = np.random.default_rng(12)
    ses = M.random_keys(rng, R.random_session(rng, 2, 640, 0))
    h = HostSrtp(host, ses, roc0={0: 2})
    state = M.new_state(ses, {0: 2})
    base = 2 << 16
    calls = [[base + 65530, base + 65533], [base + 65535, base + 65536 + 1, base + 65534], [base + 65536 + 3, base + 65532, base + 65536], [base + 65536 + 30000],
             [base + 65536 + 60000, base + 65536 + 29999], [base + 65536 + 3]]          # the last: more than 2^15 behind, its counter is guessed wrong
    for k, idx in enumerate(calls):
        dg, wire = lay_out(rng, stream_of_packets(rng, ses, 0, idx))
        want, seq = M.model_unprotect(ses, state, dg, wire), M.sequential_unprotect(ses, state, dg, wire)
        out, cnt = h.unprotect(dg, wire)
        assert cnt == want["count"] == seq["count"] and np.array_equal(wire, want["wire"]) and np.array_equal(out, want["dgrams"]), k
        assert want["state"] == seq["state"]
        state = want["state"]
        assert h.rx_index([0])[0] == state[0]["index"] == max(max(c) for c in calls[:min(k, 4) + 1])
        assert cnt["ok"] == (len(idx) if k < 5 else 0) and cnt["auth_failed"] == (0 if k < 5 else 1)
    h.close()


def test_batch_receiver_equals_sequential(host):
    """random arrival orders of sets that span fewer than 2^15 sequence numbers: verdicts and final index of the batch receiver (model and
    host form) equal the RFC's sequential receiver"""
    rng = np.random.default_rng(21)
    ses = M.random_keys(rng, R.random_session(rng, 3, 640, 0))
    crossed = False
    for trial in range(12):
        roc0 = {s: int(rng.integers(0, 4)) for s in range(3)}
        h = HostSrtp(host, ses, roc0=roc0)
        state = M.new_state(ses, roc0)
        start = {s: (roc0[s] << 16) | int(rng.choice([5, 20000, 33000])) for s in range(3)}
        for call in range(4):
            dgs = []
            for s in range(3):
                if state[s]["index"] < 0:                             # the first call: one rollover counter, the initial one
                    idx = start[s] + rng.choice(int(rng.choice([40, 3000, 32000])), size=12, replace=False)
                else:                                                 # later: within 16000 of the receiver's index, either side
                    idx = np.unique(np.maximum(state[s]["index"] + rng.integers(-16000, 16000, 12), 0))
                dgs += stream_of_packets(rng, ses, s, [int(i) for i in idx])
            dgs = [dgs[i] for i in rng.permutation(len(dgs))]
            dgs[3] = dgs[3][:20] + bytes([dgs[3][20] ^ 1]) + dgs[3][21:]
            dg, wire = lay_out(rng, dgs)
            want, seq = M.model_unprotect(ses, state, dg, wire), M.sequential_unprotect(ses, state, dg, wire)
            assert want["verdicts"] == seq["verdicts"] and want["state"] == seq["state"] and np.array_equal(want["wire"], seq["wire"]), (trial, call)
            out, cnt = h.unprotect(dg, wire)
            assert cnt == want["count"] and cnt["auth_failed"] == 1 and np.array_equal(wire, want["wire"]) and np.array_equal(out, want["dgrams"])
            crossed = crossed or any(want["state"][s]["index"] >> 16 > roc0[s] for s in range(3))
            state = want["state"]
            assert h.rx_index() == [state[s]["index"] for s in range(3)]
        h.close()
    assert crossed                                                    # some stream did pass 65535 / 0


# ---- pack's trailer ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_level", [False, True])
def test_pack_trailer(host, with_level):
    rng = np.random.default_rng(60 + with_level)
    ses = R.random_session(rng, 12, 640, 9, unbound=(3, 8))
    ses["srtp"] = {}
    n, pool_bytes = 600, 4001
    pool = rng.integers(0, 256, pool_bytes, dtype=np.uint8)
    rec = R.random_records(rng, ses, n, pool_bytes, seq_hi=2 ** 31)
    level = rng.integers(0, 256, (12, 5), dtype=np.uint8) if with_level else None
    h = HostSrtp(host, ses)
    full = R.model_pack(ses, rec, n, pool, level)
    for T_ in (0, 10, 4, 16, 1):
        assert h.set_trailer(T_) == 0
        want = M.model_pack_trailer(R, ses, rec, n, pool, level, T_)
        dg, wire, c = h.pack(rec, n, pool, level)
        assert c == want["count"] and np.array_equal(dg, want["dgrams"]) and np.array_equal(wire[:c["bytes"]], want["wire"]) and (wire[c["bytes"]:] == FILL).all(), T_
        if T_ == 0:                                                   # today's bytes and counts
            assert c == full["count"] and np.array_equal(dg, full["dgrams"]) and np.array_equal(wire[:c["bytes"]], full["wire"])
        else:
            valid = dg[:, 1] > 0
            assert np.array_equal(dg[valid, 1], full["dgrams"][valid, 1]) and (dg[:, 0] % 4 == 0).all() and c["bytes_needed"] > full["count"]["bytes_needed"]
            gaps = np.diff(dg[valid, 0]) - dg[valid, 1][:-1]
            assert (gaps >= T_).all() and (gaps < T_ + 4).all()
        # the cap covers the trailer: a datagram whose trailer does not fit is not written
        k = int(np.nonzero(dg[:, 1] > 0)[0][300])
        end = int(dg[k].sum())
        for cap in (end + T_ + (-(end + T_)) % 4, end + T_ + (-(end + T_)) % 4 - 1, end):
            wc = M.model_pack_trailer(R, ses, rec, n, pool, level, T_, cap=cap)
            dgc, wirec, cc = h.pack(rec, n, pool, level, cap=cap)
            assert cc == wc["count"] and np.array_equal(dgc, wc["dgrams"]) and np.array_equal(wirec[:cc["bytes"]], wc["wire"]) and (wirec[cc["bytes"]:] == FILL).all()
            assert (tuple(dgc[k]) != (0, 0)) == (cap >= end + T_ + (-(end + T_)) % 4)
    for bad in (-1, 17, 2 ** 31 - 1):
        assert h.set_trailer(bad) == -1
    h.close()


# ---- the control plane ---------------------------------------------------------------------------------------------------------------------------------
def test_control_plane(host):
    rng = np.random.default_rng(77)
    ses = R.random_session(rng, 5, 640, 0, unbound=(4,))
    ses["srtp"] = {}
    h = HostSrtp(host, ses)
    key = [rng.integers(0, 256, 30, dtype=np.uint8).tobytes() for _ in range(5)]
    assert h.rx_index() == [-1] * 5 and h.clear_keys([0, 1]) == 0                       # nothing allocated yet
    # refusals: nothing changes
    assert h.set_keys([0], 10, tx=key[:1]) == -1                                        # the trailer (0) is smaller than the tag
    assert h.set_trailer(4) == 0 and h.set_keys([0], 10, tx=key[:1]) == -1 and h.set_keys([0], 4, tx=key[:1]) == 0
    assert h.set_trailer(3) == -1 and h.set_trailer(0) == -1 and h.set_trailer(10) == 0   # a keyed sender's tag keeps its room
    for streams, tag, kw in (([5], 10, dict(tx=key[:1])), ([-1], 10, dict(tx=key[:1])), ([1, 1], 10, dict(tx=key[:2])), ([], 10, dict(tx=[])), ([1], 8, dict(tx=key[:1])),
                             ([1], 0, dict(rx=key[:1])), ([1], 10, dict())):
        mirror = [(host.emu_srtp_mirror(h.h, s, 0), host.emu_srtp_mirror(h.h, s, 1)) for s in range(5)]
        words = [host.emu_srtp_key_words(h.h, s) for s in range(5)]
        assert h.set_keys(streams, tag, **kw) == -1, (streams, tag)
        assert mirror == [(host.emu_srtp_mirror(h.h, s, 0), host.emu_srtp_mirror(h.h, s, 1)) for s in range(5)]
        assert words == [host.emu_srtp_key_words(h.h, s) for s in range(5)]
    assert host.emu_srtp_set_keys(None if False else h.h, None, 1, None, None, None, 10) == -1
    for lst in ([5], [0, 0], []):
        assert h.clear_keys(lst) == -1
    # a direction given as NULL keeps what it had; an rx key resets the receive state with the given counter
    assert h.set_keys([0, 1], 10, rx=key[2:4], roc=[3, 4]) == 0
    assert [host.emu_srtp_mirror(h.h, 0, w) for w in (0, 1)] == [4, 10] and [host.emu_srtp_mirror(h.h, 1, w) for w in (0, 1)] == [0, 10]
    ses["srtp"] = {0: dict(tx=key[0], rx=key[2], tag=10), 1: dict(tx=None, rx=key[3], tag=10)}
    pk = stream_of_packets(rng, ses, 0, [(3 << 16) | 9]) + stream_of_packets(rng, ses, 1, [(4 << 16) | 8])
    dg, wire = lay_out(rng, pk)
    assert h.unprotect(dg, wire)[1]["ok"] == 2 and h.rx_index([0, 1]) == [(3 << 16) | 9, (4 << 16) | 8]
    assert h.set_keys([0], 10, tx=key[4:5]) == 0 and h.rx_index([0])[0] == (3 << 16) | 9      # a tx key alone leaves the receive state
    assert h.set_keys([0], 10, rx=key[2:3]) == 0 and h.rx_index([0])[0] == -1                  # the same rx key again: "none yet", counter 0
    # clear_keys, and unbind: keys, mirror and receive state go
    assert h.clear_keys([1]) == 0 and host.emu_srtp_key_words(h.h, 1) == 0 and h.rx_index([1]) == [-1] and host.emu_srtp_mirror(h.h, 1, 1) == 0
    assert host.emu_srtp_key_words(h.h, 0) > 100
    assert h.unbind([0]) == 0 and host.emu_srtp_key_words(h.h, 0) == 0 and [host.emu_srtp_mirror(h.h, 0, w) for w in (0, 1)] == [0, 0]
    dg, wire = lay_out(rng, pk)
    assert h.unprotect(dg, wire)[1] == dict(count_dict([0] * 8), unknown_ssrc=1, no_key=1)
    assert h.set_trailer(0) == 0                                     # no keyed sender is left
    h.close()


# ---- ABI, binding ----------------------------------------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_listed_and_bound():
    import solo_amd
    hdr = T.header_text()
    lib = T.built_library()
    for name in SRTP_SYMBOLS:
        assert name in solo_amd.ABI_SYMBOLS and (name + "(") in hdr.replace(" (", "("), name
        assert hasattr(lib, name), name
    assert "#define SOLO_SRTP_MASTER_BYTES 30" in hdr and solo_amd.SRTP_MASTER_BYTES == 30
    assert C.sizeof(solo_amd.solo_srtp_count_t) == 32 and "solo_srtp_count_t;" in hdr
    assert [f for f, _ in solo_amd.solo_srtp_count_t._fields_][:6] == list(M.VERDICTS)
    bound = solo_amd.load_library()
    assert len(bound.solo_srtp_protect.argtypes) == 9 and len(bound.solo_srtp_unprotect.argtypes) == 8 and len(bound.solo_srtp_set_keys.argtypes) == 8
    assert bound.solo_srtp_protect.argtypes[6] is C.c_int64 and bound.solo_srtp_unprotect.argtypes[4] is C.c_int64
    for m in ("set_trailer", "set_keys", "clear_keys", "rx_index", "protect", "unprotect", "srtp_count"):
        assert callable(getattr(solo_amd.Rtp, m)), m
    src = open(os.path.join(T.ROOT, "solo_amd", "csrc", "solo_srtp.h")).read()
    assert "static_assert(sizeof(SxSrtpCount) == 32" in src and "sizeof(SxSrtpKey) == 256" in src


def test_capture_claims_name_a_test():
    """the header calls solo_srtp_protect and solo_srtp_unprotect capturable: tests/test_gpu_srtp.py names the test that captures each"""
    import ast
    import re
    import test_gpu_srtp as GPU
    m = re.search(r"/\* SRTP at both ends.*?\*/", open(os.path.join(T.ROOT, "include", "solo_mi355x.h")).read(), flags=re.S)
    assert m and m.group(0).count("capturable") >= 3
    tests = {n.name for n in ast.parse(open(GPU.__file__).read()).body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}
    assert set(GPU.CAPTURED) == {"solo_srtp_protect", "solo_srtp_unprotect"} and set(GPU.CAPTURED.values()) <= tests


def test_binding_checks():
    import solo_amd
    torch = pytest.importorskip("torch")
    o = object.__new__(solo_amd.Rtp)
    o.n_rows = o.n_streams = 8
    o.packet_samples, o.level_id, o.trailer = 640, 0, 4
    o.torch, o.lib, o.h, o.device = torch, T.NoLib(), None, torch.device("cpu")
    o._stream = lambda: None
    k = bytes(30)
    for bad in (-1, 17):
        with pytest.raises(ValueError):
            o.set_trailer(bad)
    for kw in (dict(streams=[0, 0], tx=[k, k], tag_bytes=4), dict(streams=[8], tx=[k], tag_bytes=4), dict(streams=[0], tx=[k[:29]], tag_bytes=4), dict(streams=[0], tag_bytes=4),
               dict(streams=[0], tx=[k], tag_bytes=8), dict(streams=[0], tx=[k], tag_bytes=10), dict(streams=[0, 1], rx=[k], tag_bytes=4),
               dict(streams=[0], rx=[k], rx_roc=2 ** 32), dict(streams=[0], rx=[k], rx_roc=[1, 2])):
        with pytest.raises(ValueError):
            o.set_keys(**kw)
    for lst in ([], [8], [0, 0]):
        with pytest.raises(ValueError):
            o.clear_keys(lst)
        with pytest.raises(ValueError):
            o.rx_index(lst)
    D = T.FakeDev
    I32, U8 = torch.int32, torch.uint8
    good = dict(records=D((10, 5), I32), send_count=D((8,), I32), dgrams=D((10, 2), I32), wire=D((999,), U8))
    for over in (dict(records=D((10, 4), I32)), dict(records=D((0, 5), I32), dgrams=D((0, 2), I32)), dict(send_count=D((6,), I32)), dict(dgrams=D((9, 2), I32)),
                 dict(dgrams=None), dict(wire=D((999,), I32)), dict(wire=D((999,), U8, cuda=False)), dict(wire=D((999,), U8, contiguous=False))):
        with pytest.raises(ValueError):
            o.protect(**dict(good, **over))
    good = dict(dgrams=D((10, 2), I32), wire=D((999,), U8), dgrams_out=D((10, 2), I32))
    for over in (dict(dgrams=D((10, 3), I32)), dict(wire=D((9, 9), U8)), dict(dgrams_out=D((9, 2), I32)), dict(dgrams_out=D((10, 2), I32, cuda=False)), dict(wire=None)):
        with pytest.raises(ValueError):
            o.unprotect(**dict(good, **over))


# ---- the built library's kernels ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="no LLVM binutils on this box")
def test_srtp_kernels_use_no_scratch():
    import solo_amd
    T.built_library()
    sys.path.insert(0, os.path.join(T.ROOT, "tools"))
    from kernel_resources import kernel_resources
    seen = kernel_resources(solo_amd.LIB_PATH)
    for frag in KERNELS:
        hits = [r for name, r in seen.items() if frag in name]
        assert len(hits) == 1, (frag, len(hits))
        assert hits[0]["scratch"] == 0, (frag, hits[0])


# ---- the same source as a stand-alone program under the sanitisers ---------------------------------------------------------------------------------------
def test_stand_alone_build_under_the_sanitisers(tmp_path):
    """tests/srtp_host.cpp with its own main, -fsanitize=address,undefined: the hostile family in through a file, in heap blocks of exactly
    their size, every output back through a file and against the model; any report of a sanitiser ends the program with a non-zero status"""
    exe = str(tmp_path / "srtp_asan")
    flags = [f for f in FLAGS if f not in ("-shared", "-fPIC", "-O2")] + ["-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                                                         "-DSRTP_MAIN"]
    cxx = os.environ.get("CXX", "g++")
    if os.path.basename(cxx).startswith("g++"):                       # the runtimes inside the program: nothing has to load ahead of it
        flags += ["-static-libasan", "-static-libubsan"]
    subprocess.check_call([cxx] + flags + [source("srtp"), "-o", exe])
    for tag in (10, 4):
        rng = np.random.default_rng(500 + tag)
        ses = R.random_session(rng, 6, 640, 5)
        M.random_keys(rng, ses, tag)
        roc0 = {s: 7 * s for s in range(6)}
        state = M.new_state(ses, roc0)
        kinds = M.hostile_set(ses, state, 2, rng, R) + M.hostile_set(ses, state, 5, rng, R)
        dg, wire = lay_out(rng, [k[1] for k in kinds], front=0, gap=0)
        wire = wire[:int(dg[-1].sum())]                               # the last datagram ends with the block
        dg = np.concatenate([dg, np.array([[wire.size - 10, 40], [-4, 30], [wire.size, 16]], np.int32)])
        want = M.model_unprotect(ses, state, dg, wire)
        assert want["verdicts"][:len(kinds)] == [k[2] for k in kinds]
        fin, fout = str(tmp_path / ("in%d.bin" % tag)), str(tmp_path / ("out%d.bin" % tag))
        with open(fin, "wb") as f:
            f.write(np.array([6, dg.shape[0], wire.size, tag, 0, 0, 0, 0], np.int32).tobytes())
            f.write(np.array([ses["streams"][s]["ssrc"] for s in range(6)], np.uint32).tobytes())
            f.write(np.array([roc0[s] for s in range(6)], np.uint32).tobytes())
            f.write(b"".join(ses["srtp"][s]["rx"] for s in range(6)))
            f.write(dg.tobytes())
            f.write(wire.tobytes())
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        raw = open(fout, "rb").read()
        n = dg.shape[0]
        out = np.frombuffer(raw[:8 * n], np.int32).reshape(n, 2)
        cnt = np.frombuffer(raw[8 * n:8 * n + 32], np.int32)
        index = np.frombuffer(raw[8 * n + 32:8 * n + 32 + 48], np.int64)
        w = np.frombuffer(raw[8 * n + 80:], np.uint8)
        assert count_dict(cnt) == want["count"] and np.array_equal(out, want["dgrams"]) and np.array_equal(w, want["wire"])
        assert index.tolist() == [want["state"][s]["index"] for s in range(6)]

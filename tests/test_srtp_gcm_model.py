"""AEAD_AES_128_GCM in the SRTP and the SRTCP stage (RFC 7714; solo_amd/csrc/solo_srtp_gcm.h) without a GPU.  The independent model of
tests/srtp_gcm_model.py is pinned to the published answers (the GCM specification's cases 1 - 4, RFC 7714 sections 16.1.1, 16.2.1, 16.2.2),
to the fixture tests/golden/srtp_gcm_cases.npz that the system's libcrypto made, and to fresh random cases where libcrypto loads.  The
compiled side (tests/srtp_gcm_host.cpp through tests/host_build.py: the table multiplication, GHASH, the cipher, key derivation, the host
forms of the four calls in sessions of both transforms, the control plane) is compared byte for byte with the model.  Then the binding's
checks, the ABI, the built library's new kernels (no scratch), and the hostile family once more through a stand-alone build of the same
source under the address and undefined-behaviour sanitisers."""
import ctypes as C
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

import rtcp_model as RC
import rtp_model as R
import solo_testlib as T
import srtcp_model as CM
import srtp_gcm_model as G
import srtp_model as S
import test_srtcp_model as TC
import test_srtp_model as TS
from host_build import FLAGS, host_lib, source

sys.path.insert(0, T.GOLDEN)
import make_srtp_gcm_golden as LC      # noqa: E402

H = bytes.fromhex
p = TS.p
KERNELS = ("solo_srtp_gcm_protect_kernel", "solo_srtp_gcm_unprotect_kernel", "solo_srtcp_gcm_protect_kernel", "solo_srtcp_gcm_unprotect_kernel")
OLD_KERNELS = TS.KERNELS + TC.KERNELS
VP, I, LL, U = C.c_void_p, C.c_int, C.c_longlong, C.c_uint

# ---- published answers ------------------------------------------------------------------------------------------------------------------------------
K3, IV3 = H("feffe9928665731c6d6a8f9467308308"), H("cafebabefacedbaddecaf888")
P3 = H("d9313225f88406e5a55909c5aff5269a86a7a9531534f7da2e4c303d8a318a721c3c0c95956809532fcf0e2449a6b525b16aedf5aa0de657ba637b391aafd255")
C3 = H("42831ec2217774244b7221b784d0d49ce3aa212f2c02a4e035c17e2329aca12e21d514b25466931c7d8f6a5aac84aa051ba30b396a0aac973d58e091473f5985")
A4 = H("feedfacedeadbeeffeedfacedeadbeefabaddad2")
SPEC = [(bytes(16), bytes(12), b"", b"", b"", H("58e2fccefa7e3061367f1d57a4e7455a")),
        (bytes(16), bytes(12), b"", bytes(16), H("0388dace60b6a392f328c2b971b2fe78"), H("ab6e47d42cec13bdf53a67b21257bddf")),
        (K3, IV3, b"", P3, C3, H("4d5c2af327cd64a62cf35abd2ba6fab4")),
        (K3, IV3, A4, P3[:60], C3[:60], H("5bc94fbc3221a5db94fae95ae7121a47"))]
RFC_KEYS = dict(ke=H("000102030405060708090a0b0c0d0e0f"), ks=H("517569642070726f2071756f"))
RFC_RTP = H("8040f17b8041f8d35501a0b2") + b"Gallia est omnis divisa in partes tres"
RFC_SRTP = RFC_RTP[:12] + H("f24de3a3fb34de6cacba861c9d7e4bcabe633bd50d294e6f42a5f47a51c7d19b36de3adf8833") + H("899d7f27beb16a9152cf765ee4390cce")
RFC_RTCP = H("81c8000d4d6172734e5450314e545032525450200000042a0000e9304c756e61") + H("deadbeef") * 5
RFC_SRTCP = RFC_RTCP[:8] + H("63e94885dcdab67ca727d7662f6b7e997ff5c0f76c06f32dc676a5f1730d6fda4ce09b4686303ded0bb9275b") + H("c84aa45896cf4d2fc5abf87245d9eade") + \
    H("800005d4")
RFC_SRTCP_E0 = RFC_RTCP + H("841dd9683dd78ec92ae58790125f62b3") + H("000005d4")


@pytest.fixture(scope="module")
def fixture():
    z = np.load(os.path.join(T.GOLDEN, "srtp_gcm_cases.npz"))

    def items(name):
        blob, off = z[name + "_blob"], z[name + "_off"]
        return [blob[off[i]:off[i + 1]].tobytes() for i in range(len(off) - 1)]
    cases = list(zip((k.tobytes() for k in z["key"]), (v.tobytes() for v in z["iv"]), items("aad"), items("pt"), items("ct"), (t.tobytes() for t in z["tag"])))
    srtp = list(zip((k.tobytes() for k in z["srtp_ke"]), (k.tobytes() for k in z["srtp_ks"]), z["srtp_meta"].tolist(), items("srtp_plain"), items("srtp_wire")))
    srtcp = list(zip((k.tobytes() for k in z["srtcp_ke"]), (k.tobytes() for k in z["srtcp_ks"]), z["srtcp_meta"].tolist(), items("srtcp_plain"), items("srtcp_wire")))
    return dict(cases=cases, srtp=srtp, srtcp=srtcp)


def test_model_published_answers():
    for k, iv, a, pt, ct, tag in SPEC:
        assert G.gcm_encrypt(k, iv, a, pt) == (ct, tag) and G.gcm_decrypt(k, iv, a, ct, tag) == pt
    assert G.rtp_iv(RFC_KEYS["ks"], 0x5501a0b2, 0, 0xf17b) == H("51753c6580c2726f20718414")
    assert G.protect_packet(RFC_KEYS, RFC_RTP, 0) == RFC_SRTP
    assert G.rtcp_iv(RFC_KEYS["ks"], 0x4d617273, 0x5d4) == H("517524055203726f207170bb")
    assert G.protect_rtcp_packet(RFC_KEYS, RFC_RTCP, 0x5d4) == RFC_SRTCP and G.protect_rtcp_packet(RFC_KEYS, RFC_RTCP, 0x5d4, e=0) == RFC_SRTCP_E0
    assert G.unprotect_rtcp_packet(RFC_KEYS, RFC_SRTCP) == (True, RFC_RTCP, 0x5d4) and G.unprotect_rtcp_packet(RFC_KEYS, RFC_SRTCP_E0) == (True, RFC_RTCP, 0x5d4)
    # the field: H . 1 = H, and multiplying by x is the right shift with R folded in
    one, x = 1 << 127, 1 << 126
    assert G.gf_mul(0x1234 << 100 | 1, one) == (0x1234 << 100 | 1) and G.gf_mul(1, x) == G.R and G.gf_mul(x, x) == 1 << 125


def test_model_against_the_fixture(fixture):
    assert len(fixture["cases"]) == 3 * len(LC.AAD_LENGTHS) * len(LC.PT_LENGTHS)
    assert {(len(c[2]), len(c[3])) for c in fixture["cases"]} == {(a, n) for a in LC.AAD_LENGTHS for n in LC.PT_LENGTHS} and G.LENGTHS == LC.PT_LENGTHS
    for k, iv, a, pt, ct, tag in fixture["cases"]:
        assert G.gcm_encrypt(k, iv, a, pt) == (ct, tag)
    for ke, ks, (ssrc, roc, seq, hdr), plain, wire in fixture["srtp"]:
        assert G.protect_packet(dict(ke=ke, ks=ks), plain, roc) == wire and S.header_bytes(plain) == hdr
    for ke, ks, (ssrc, index, e), plain, wire in fixture["srtcp"]:
        assert G.protect_rtcp_packet(dict(ke=ke, ks=ks), plain, index, e) == wire
        assert G.unprotect_rtcp_packet(dict(ke=ke, ks=ks), wire) == (True, plain, index)


@pytest.mark.skipif(LC.libcrypto() is None, reason="no libcrypto on this box")
def test_model_against_libcrypto_on_fresh_cases():
    seed = int.from_bytes(os.urandom(4), "little")
    print("seed %d" % seed)                                           # (shown with a failure: np.random.default_rng(seed) gives the cases again)
    rng = np.random.default_rng(seed)
    for _ in range(40):
        k, iv = rng.integers(0, 256, 16, dtype=np.uint8).tobytes(), rng.integers(0, 256, 12, dtype=np.uint8).tobytes()
        a, pt = (rng.integers(0, 256, int(rng.integers(0, n)), dtype=np.uint8).tobytes() for n in (50, 200))
        assert G.gcm_encrypt(k, iv, a, pt) == LC.gcm(k, iv, a, pt), (seed, k.hex(), iv.hex(), a.hex(), pt.hex())


# ---- the compiled pieces -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host():
    lib = host_lib("srtp_gcm")
    lib.emu_srtp_create.restype = VP
    lib.emu_srtp_create.argtypes = [I, I]
    lib.emu_srtp_destroy.argtypes = [VP]
    lib.emu_srtp_bind.argtypes = [VP, VP, I] + [VP] * 5 + [I]
    lib.emu_srtp_unbind.argtypes = [VP, VP, I]
    lib.emu_srtp_set_trailer.argtypes = [VP, I]
    lib.emu_srtp_set_keys.argtypes = [VP, VP, I, VP, VP, VP, I]
    lib.emu_srtp_clear_keys.argtypes = [VP, VP, I]
    lib.emu_srtp_rx_index.argtypes = [VP, VP, I, VP]
    lib.emu_srtp_mirror.argtypes = [VP, I, I]
    lib.emu_srtp_key_words.argtypes = [VP, I]
    lib.emu_srtp_pack.argtypes = [VP, VP, VP, I, VP, LL, VP, I, VP, VP, LL, VP]
    lib.emu_srtcp_create.restype = VP
    lib.emu_srtcp_create.argtypes = [VP, I]
    lib.emu_srtcp_destroy.argtypes = [VP]
    lib.emu_srtcp_unbind.argtypes = [VP, VP, I]
    lib.emu_srtcp_set_keys.argtypes = [VP, VP, I, VP, VP, VP, VP]
    lib.emu_srtcp_clear_keys.argtypes = [VP, VP, I]
    lib.emu_srtcp_get_index.argtypes = [VP, VP, I, VP, VP]
    lib.emu_srtcp_snapshot.argtypes = [VP, VP]
    lib.emu_srtcp_key_words.argtypes = [VP, I]
    lib.emu_gcm_mul.argtypes = [VP, VP, I, VP]
    lib.emu_gcm_ghash.argtypes = [VP, VP, I, U, I, VP, I, VP]
    lib.emu_gcm_encrypt.argtypes = [VP, VP, VP, I, VP, I, VP]
    lib.emu_gcm_derive.argtypes = [VP, I, VP, VP, VP]
    lib.emu_gcm_srtp_set_keys.argtypes = [VP, VP, I, VP, VP, VP]
    lib.emu_gcm_srtp_set_session.argtypes = [VP, I, I, VP, VP, U]
    lib.emu_gcm_srtp_record.argtypes = [VP, I, I, VP]
    lib.emu_gcm_srtp_any.argtypes = [VP, I]
    lib.emu_gcm_srtp_protect.argtypes = [VP, VP, VP, I, VP, VP, LL, VP]
    lib.emu_gcm_srtp_unprotect.argtypes = [VP, VP, I, VP, LL, VP, VP]
    lib.emu_gcm_srtcp_set_keys.argtypes = [VP, VP, I, VP, VP, VP, VP]
    lib.emu_gcm_srtcp_set_session.argtypes = [VP, I, I, VP, VP, LL]
    lib.emu_gcm_srtcp_record.argtypes = [VP, I, I, VP]
    lib.emu_gcm_srtcp_mirror.argtypes = [VP, I, I]
    lib.emu_gcm_srtcp_protect.argtypes = [VP, I, I, VP, I, VP, VP, VP, LL, VP]
    lib.emu_gcm_srtcp_unprotect.argtypes = [VP, VP, I, VP, LL, VP, VP]
    # the sessions of the two older test files run through this library's calls: the four device calls as solo_api.hip issues them
    lib.emu_srtp_protect.argtypes = [VP, VP, VP, I, VP, VP, LL, VP]
    lib.emu_srtp_unprotect.argtypes = [VP, VP, I, VP, LL, VP, VP]
    lib.emu_srtcp_protect.argtypes = [VP, I, I, VP, I, VP, VP, VP, LL, VP]
    lib.emu_srtcp_unprotect.argtypes = [VP, VP, I, VP, LL, VP, VP]
    lib.alone = {name: getattr(lib, "emu_%s" % name) for name in ("srtp_protect", "srtp_unprotect", "srtcp_protect", "srtcp_unprotect")}    # the older pass ALONE
    lib.emu_srtp_protect, lib.emu_srtp_unprotect = lib.emu_gcm_srtp_protect, lib.emu_gcm_srtp_unprotect
    lib.emu_srtcp_protect, lib.emu_srtcp_unprotect = lib.emu_gcm_srtcp_protect, lib.emu_gcm_srtcp_unprotect
    return lib


def buf(b):
    return np.frombuffer(bytes(b), np.uint8).copy()


def host_mul(host, h, x, stride=1):
    out, hh, xx = np.zeros(16, np.uint8), buf(h.to_bytes(16, "big")), buf(x.to_bytes(16, "big"))
    host.emu_gcm_mul(p(hh), p(xx), stride, p(out))
    return int.from_bytes(out.tobytes(), "big")


def test_host_multiplication_equals_the_model(host):
    """the table multiplication against the bit-serial one: the single-bit operands on either side reach every table entry (each is a sum
    of the four multiples a single bit selects) and every reduction constant"""
    rng = np.random.default_rng(128)
    rnd = [int.from_bytes(rng.integers(0, 256, 16, dtype=np.uint8).tobytes(), "big") for _ in range(24)]
    special = [0, 1 << 127, (1 << 128) - 1, 1, G.R]
    bits = [1 << k for k in range(128)]
    for h in special + rnd[:4]:
        for x in special + bits + rnd[4:12]:
            assert host_mul(host, h, x) == G.gf_mul(x, h), (hex(h), hex(x))
    for h in bits:
        for x in special + rnd[12:16] + [bits[(3 * k + 1) % 128] for k in range(4)]:
            assert host_mul(host, h, x) == G.gf_mul(x, h), (hex(h), hex(x))
    for h, x in zip(rnd[:12], rnd[12:]):                               # the tile's layout: [entry][word][lane], the last lane of 64
        assert host_mul(host, h, x, 64) == G.gf_mul(x, h) and G.gf_mul(x, h) == G.gf_mul(h, x)
    # every nibble value at every nibble position against every reduction constant: x = e << 4k under an H whose low bits are set
    h = rnd[16] | 0xF
    for k in range(32):
        for e in range(16):
            assert host_mul(host, h, e << (4 * k)) == G.gf_mul(e << (4 * k), h), (k, e)


def test_host_ghash_and_gcm_against_the_fixture(host, fixture):
    out, tag = np.zeros(16, np.uint8), np.zeros(16, np.uint8)
    for n, (k, iv, a, pt, ct, t) in enumerate(SPEC + fixture["cases"]):
        al = n % 4                                                     # message and associated data at every alignment
        ab, cb = np.zeros(len(a) + 8, np.uint8), np.zeros(len(pt) + 8, np.uint8)
        a0, c0 = (al - ab.ctypes.data) % 4, ((al + 1) - cb.ctypes.data) % 4
        aa, cc = ab[a0:a0 + len(a)], cb[c0:c0 + len(pt)]
        aa[:], cc[:] = buf(a), buf(ct)
        hk = buf(S.aes_encrypt(k, bytes(16)))
        host.emu_gcm_ghash(p(hk), p(aa), len(a), 0, 0, p(cc), len(ct), p(out))
        assert out.tobytes() == G.ghash(hk.tobytes(), a, ct), n
        cc[:] = buf(pt)
        kk, vv = buf(k), buf(iv)
        host.emu_gcm_encrypt(p(kk), p(vv), p(aa), len(a), p(cc), len(pt), p(tag))
        assert (cc.tobytes(), tag.tobytes()) == (ct, t), n
        assert not ab[:a0].any() and not ab[a0 + len(a):].any() and not cb[:c0].any() and not cb[c0 + len(pt):].any()
    # the word behind the associated data (SRTCP), at the lengths that put it across a block edge
    rng = np.random.default_rng(5)
    hk = rng.integers(0, 256, 16, dtype=np.uint8)
    for n_a in (0, 3, 8, 12, 13, 15, 16, 28, 29):
        a, ct = rng.integers(0, 256, n_a, dtype=np.uint8), rng.integers(0, 256, 21, dtype=np.uint8)
        host.emu_gcm_ghash(p(hk), p(a), n_a, 0x800005D4, 4, p(ct), 21, p(out))
        assert out.tobytes() == G.ghash(hk.tobytes(), a.tobytes() + H("800005d4"), ct.tobytes()), n_a


def test_host_key_derivation_equals_the_model(host):
    rng = np.random.default_rng(2)
    for master in (bytes(range(28)), G.random_master(rng), G.random_master(rng)):
        for label in (0, 3):
            ke, ks, rec, m = np.zeros(16, np.uint8), np.zeros(12, np.uint8), np.zeros(64, np.uint32), buf(master)
            host.emu_gcm_derive(p(m), label, p(ke), p(ks), p(rec))
            want = G.session_keys(master, label)
            assert (ke.tobytes(), ks.tobytes()) == (want["ke"], want["ks"])
            # the record: round keys (the first four are the key), the 12 salt bytes, H where the HMAC state was, tag 16, has, transform
            assert rec[:4].astype(">u4").tobytes() == want["ke"] and rec[44:47].astype(">u4").tobytes() == want["ks"] and rec[47] == 0
            assert rec[48:52].astype(">u4").tobytes() == S.aes_encrypt(want["ke"], bytes(16)) and not rec[52:58].any()
            assert rec[58:64].tolist() == [16, 1, 1, 0, 0, 0]
        # the padded salt: the PRF of RFC 3711 over master key || salt || 00 00, and the two stages' keys differ
        assert G.session_keys(master, 0)["ke"] == S.derive(master[:16], master[16:] + b"\0\0", 0, 16) != G.session_keys(master, 3)["ke"]
    assert [host.emu_gcm_sizes(k) for k in range(5)] == [16, 20, 28, 64, 256]


# ---- SRTP: the host forms in sessions of both transforms ---------------------------------------------------------------------------------------------
class HostGcm(TS.HostSrtp):
    """tests/test_srtp_model.py's session, with tag 16 meaning a GCM key"""

    def set_keys(self, streams, tag, tx=None, rx=None, roc=None):
        if tag != G.TAG:
            return super().set_keys(streams, tag, tx, rx, roc)
        s = np.array(streams, np.int32)
        txa = None if tx is None else np.frombuffer(b"".join(tx), np.uint8)
        rxa = None if rx is None else np.frombuffer(b"".join(rx), np.uint8)
        ra = None if roc is None else np.array(roc, np.uint32)
        return self.lib.emu_gcm_srtp_set_keys(self.h, p(s), len(streams), p(txa), p(rxa), p(ra))


def cm_entry(rng, tag):
    return dict(tx=rng.integers(0, 256, 30, dtype=np.uint8).tobytes(), rx=rng.integers(0, 256, 30, dtype=np.uint8).tobytes(), tag=tag)


def mixed_session(rng, level_id):
    """6 streams: 0 and 1 GCM, 2 AES-CM / HMAC-80, 3 AES-CM / HMAC-32, 4 bound without a key, 5 not bound"""
    ses = R.random_session(rng, 6, 640, level_id, unbound=(5,))
    ses["srtp"] = {0: G.gcm_entry(rng), 1: G.gcm_entry(rng), 2: cm_entry(rng, 10), 3: cm_entry(rng, 4)}
    return ses


def protect_case(rng, with_level):
    """every plaintext length under GCM and some under AES-CM; stream 0's indices around the 16-bit wrap (seq_offset 65534: ROC 0 and 1
    inside one packet's two descriptions), stream 1's at the mod-2^32 edge; a record of the keyless, of the unbound stream, a bad desc"""
    ses = mixed_session(rng, 3)
    ses["streams"][0]["seq_offset"], ses["streams"][1]["seq_offset"] = 65534, 65535
    rec, at = [], 0
    for i, ln in enumerate(G.LENGTHS[1:]):
        rec.append([i % 2, 100 + i, i % 2, at, ln])
        rec.append([2 + i % 2, 100 + i, i % 2, at, ln])
        at += ln
    rec += [[0, 0, 0, 3, 40], [0, 0, 1, 5, 41], [0, 1, 0, 7, 42], [1, 2 ** 31 - 1, 0, 11, 44], [1, 2 ** 31 - 1, 1, 13, 45], [4, 7, 0, 0, 30], [5, 7, 0, 0, 30], [0, 8, 2, 0, 30]]
    rec = np.array(rec, np.int32)
    pool = rng.integers(0, 256, at + 300, dtype=np.uint8)
    level = rng.integers(0, 255, (6, 4), dtype=np.uint8) if with_level else None
    return ses, rec, pool, level


@pytest.mark.parametrize("with_level", [False, True])
def test_host_protect_against_model(host, with_level):
    rng = np.random.default_rng(160 + with_level)
    ses, rec, pool, level = protect_case(rng, with_level)
    h = HostGcm(host, ses)
    n, Hb = rec.shape[0], 20 if with_level else 12
    dg, wire, c = h.pack(rec, n, pool, level)
    want_pack = S.model_pack_trailer(R, ses, rec, n, pool, level, 16)
    assert c == want_pack["count"] and c["refused"] == 2 and np.array_equal(dg, want_pack["dgrams"])
    packed_dg, packed = dg.copy(), wire.copy()
    want = G.model_protect(ses, rec, n, dg, wire)
    got = h.protect(rec, n, dg, wire)
    assert got == want["count"] and got == dict(want["count"], ok=n - 3, skipped=2, no_key=1, malformed=0, unknown_ssrc=0, auth_failed=0, reserved0=0, reserved1=0)
    assert np.array_equal(dg, want["dgrams"]) and np.array_equal(wire, want["wire"])
    live = dg[:, 1] > 0
    grown = np.array([{0: 16, 1: 16, 2: 10, 3: 4}.get(int(s), 0) for s in rec[:, 0]])
    assert (dg[live, 1] == packed_dg[live, 1] + grown[live]).all() and tuple(dg[n - 3]) == (0, 0) and tuple(packed_dg[n - 3]) != (0, 0)
    # the rollover counters of the wrap records, and the header (with the level in it) left readable under either transform
    for k, roc in ((n - 8, 0), (n - 7, 0), (n - 6, 1), (n - 5, 65536), (n - 4, 65536)):
        off, ln = packed_dg[k]
        sp = G.protect_packet(G.session_keys(ses["srtp"][int(rec[k, 0])]["tx"]), packed[off:off + ln].tobytes(), roc)
        assert wire[off:off + ln + 16].tobytes() == sp, k
    for k in np.nonzero(live)[0]:
        off = dg[k, 0]
        assert np.array_equal(wire[off:off + Hb], packed[off:off + Hb])
        if packed_dg[k, 1] - Hb >= 15:
            assert not np.array_equal(wire[off + Hb:off + packed_dg[k, 1]], packed[off + Hb:off + packed_dg[k, 1]])
    # loopback through the receiving end, fed per rollover counter
    rx = HostGcm(host, G.loop_session(ses), roc0={0: 1, 1: 1})        # (65534 + 2 x 100 and more: the senders stand behind their first wrap)
    for sel in (np.nonzero(live & (rec[:, 1] >= 100) & (rec[:, 1] < 1000))[0], [n - 8, n - 7], [n - 6], [n - 5, n - 4]):
        sub = dg[list(sel)]
        w2 = wire.copy()
        if list(sel) == [n - 5, n - 4]:
            rx.set_keys([1], 16, rx=[ses["srtp"][1]["tx"]], roc=[65536])
        out, cu = rx.unprotect(sub, w2)
        assert cu["ok"] == len(sub), (sel, cu)
        assert np.array_equal(out[:, 0], sub[:, 0]) and np.array_equal(out[:, 1], packed_dg[list(sel), 1])
        for (off, ln) in out:
            assert np.array_equal(w2[off:off + ln], packed[off:off + ln])
    # a refused list; a cut by max_records; a tag that would reach past wire_bytes
    dg2, w2 = packed_dg.copy(), packed.copy()
    assert h.protect(rec, -1, dg2, w2) == dict(want["count"], ok=-1, skipped=0, no_key=0) and np.array_equal(dg2, packed_dg) and np.array_equal(w2, packed)
    assert h.protect(rec, n, dg2, w2, max_records=5)["ok"] == 5 and np.array_equal(dg2[5:], packed_dg[5:]) and np.array_equal(dg2[:5], dg[:5])
    last = int(np.nonzero(live & (rec[:, 0] < 2))[0][-1])
    end = int(packed_dg[last].sum())
    for wb, ok in ((end + 16, True), (end + 15, False), (end - 1, False)):
        dg3, w3 = packed_dg.copy(), packed.copy()
        cm = G.model_protect(ses, rec, n, dg3.copy(), w3, wire_bytes=wb)
        got = h.protect(rec, n, dg3, w3, wire_bytes=wb)
        assert got == cm["count"] and np.array_equal(dg3, cm["dgrams"]) and np.array_equal(w3, cm["wire"])
        assert (tuple(dg3[last]) != (0, 0)) == ok and got["malformed"] >= (0 if ok else 1)
    h.close()
    rx.close()


def hostile_case(rng, align=None):
    ses = mixed_session(rng, 5)
    ses["srtp"][4] = dict(G.gcm_entry(rng), rx=None)                   # a GCM sender without an rx key
    state = S.new_state(ses, {0: 7})
    kinds = G.hostile_set(ses, state, 0, rng, R) + G.hostile_set(ses, state, 1, rng, R) + S.hostile_set(ses, state, 2, rng, R)
    # a datagram of a stream keyed for the other transform, either way round
    c0, c2 = ses["streams"][0], ses["streams"][2]
    kinds.append(("cm_on_gcm_stream", S.protect_packet(S.session_keys(bytes(30)), 10, R.build(c0["ssrc"], 96, 2000, 0, b"y" * 50), 7), "auth_failed"))
    kinds.append(("gcm_on_cm_stream", G.protect_packet(G.session_keys(ses["srtp"][0]["rx"]), R.build(c2["ssrc"], 96, 1001, 0, b"z" * 50), 0), "auth_failed"))
    kinds.append(("no_key", R.build(ses["streams"][4]["ssrc"], 96, 3, 0, b"x" * 30), "no_key"))
    order = rng.permutation(len(kinds))
    dg, wire = TS.lay_out(rng, [kinds[i][1] for i in order], front=int(rng.integers(0, 4)), align=align)
    return ses, state, [kinds[i] for i in order], dg, wire


def test_host_unprotect_verdicts_in_rule_order(host):
    for align in (0, 1, 2, 3, None):
        rng = np.random.default_rng(270 + (9 if align is None else align))
        ses, state, kinds, dg, wire = hostile_case(rng, align)
        if align is not None:
            assert (dg[:, 0] % 4 == align).all()
        want = G.model_unprotect(ses, state, dg, wire)
        assert want["verdicts"] == [k[2] for k in kinds], [(k[0], k[2], v) for k, v in zip(kinds, want["verdicts"]) if k[2] != v]
        assert set(want["verdicts"]) == {"ok", "malformed", "unknown_ssrc", "no_key", "auth_failed"}
        h = HostGcm(host, ses, roc0={0: 7})
        before = wire.copy()
        backing = np.full(wire.size + 64, 0x3C, np.uint8)              # guard bytes around the wire
        a0 = 32 + (0 - backing.ctypes.data - 32) % 4
        w = backing[a0:a0 + wire.size]
        w[:] = wire
        out, cnt = h.unprotect(dg, w)
        assert cnt == want["count"], (cnt, want["count"])
        assert np.array_equal(out, want["dgrams"]) and np.array_equal(w, want["wire"])
        assert (backing[:a0] == 0x3C).all() and (backing[a0 + wire.size:] == 0x3C).all()
        touched = np.zeros(wire.size, bool)
        for (off, ln), v in zip(out, want["verdicts"]):
            if v == "ok":
                touched[off:off + ln] = True
        assert np.array_equal(w[~touched], before[~touched]) and not np.array_equal(w[touched], before[touched])
        assert h.rx_index() == [want["state"][s]["index"] for s in range(6)] and h.rx_index([0])[0] >> 16 == 7
        # in place: d_dgrams_out may be d_dgrams, for the datagrams the older kernel leaves to this one too
        h2 = HostGcm(host, ses, roc0={0: 7})
        w2, dg2 = wire.copy(), dg.copy()
        cnt2 = np.full(8, -9, np.int32)
        host.emu_gcm_srtp_unprotect(h2.h, p(dg2), dg2.shape[0], p(w2), w2.size, p(dg2), p(cnt2))
        assert np.array_equal(dg2, want["dgrams"]) and np.array_equal(w2, want["wire"]) and TS.count_dict(cnt2) == want["count"]
        h2.close()
        # a second call continues from the first call's index: what was accepted is accepted again (no replay list), newer packets too
        state2 = want["state"]
        more = G.hostile_set(ses, state2, 0, rng, R)[:5] + S.hostile_set(ses, state2, 2, rng, R)[:3]
        dgm, wm = TS.lay_out(rng, [k[1] for k in more], align=align)
        want2 = G.model_unprotect(ses, state2, dgm, wm)
        out, cnt = h.unprotect(dgm, wm)
        assert cnt == want2["count"] and cnt["ok"] == 8 and np.array_equal(out, want2["dgrams"]) and np.array_equal(wm, want2["wire"])
        assert h.rx_index() == [want2["state"][s]["index"] for s in range(6)]
        # ranges that leave the wire are malformed and never read
        bad = np.array([[-1, 40], [wire.size - 39, 40], [wire.size, 16], [2 ** 31 - 1, 2 ** 31 - 1], [0, -5], [0, 0]], np.int32)
        out, cnt = h.unprotect(bad, w)
        assert cnt["malformed"] == 6 and not out.any() and np.array_equal(w, want["wire"])
        h.close()


def test_host_srtp_published_and_fixture_datagrams(host, fixture):
    """RFC 7714 section 16.1.1 and the fixture's libcrypto-made datagrams through the host forms: the session bound with their SSRCs and
    sequence numbers, the SESSION keys put in through the test-only path"""
    cases = [(RFC_KEYS["ke"], RFC_KEYS["ks"], (0x5501a0b2, 0, 0xf17b, 12), RFC_RTP, RFC_SRTP)] + fixture["srtp"]
    n = len(cases)
    ses = R.session(n, 640, 3, {s: dict(ssrc=int(c[2][0]), ts_offset=0, seq_offset=0, pt=(96, 97)) for s, c in enumerate(cases)})
    ses["srtp"] = {}
    h = HostGcm(host, ses, trailer=16)
    for s, (ke, ks, (ssrc, roc, seq, hdr), plain, wire) in enumerate(cases):
        for d in (0, 1):
            assert host.emu_gcm_srtp_set_session(h.h, s, d, p(buf(ke)), p(buf(ks)), roc) == 0
    rng = np.random.default_rng(3)
    dg, wire = TS.lay_out(rng, [c[4] for c in cases])
    out, cnt = h.unprotect(dg, wire)
    assert cnt == dict(TS.count_dict([0] * 8), ok=n)
    for (off, ln), c in zip(out.tolist(), cases):
        assert wire[off:off + ln].tobytes() == c[3]
    assert h.rx_index() == [(c[2][1] << 16) | c[2][2] for c in cases]
    # protect: record s of stream s with seq_offset + 2 seq + desc = the packet's index; the RTP packet laid out as pack leaves it
    h.close()
    for s, c in enumerate(cases):
        ses["streams"][s]["seq_offset"] = int(c[2][2])
    h = HostGcm(host, ses, trailer=16)
    rec = np.array([[s, (c[2][1] << 16) // 2, 0, 0, len(c[3]) - c[2][3]] for s, c in enumerate(cases) if c[2][1] < 2 ** 15], np.int32)
    sel = [int(s) for s in rec[:, 0]]
    assert 0 in sel and len(sel) >= 6
    for s in sel:
        assert host.emu_gcm_srtp_set_session(h.h, s, 0, p(buf(cases[s][0])), p(buf(cases[s][1])), 0) == 0
    dg, wire = TS.lay_out(rng, [cases[s][3] + bytes(16) for s in sel], align=0)
    dg[:, 1] -= 16
    got = h.protect(rec, len(sel), dg, wire)
    assert got == dict(TS.count_dict([0] * 8), ok=len(sel))
    for (off, ln), s in zip(dg.tolist(), sel):
        assert wire[off:off + ln].tobytes() == cases[s][4], s
    h.close()


# ---- SRTCP ---------------------------------------------------------------------------------------------------------------------------------------------
class HostRtcpSes(TC.HostSes):
    """tests/test_srtcp_model.py's session; a keys entry with gcm=True is set through the GCM call"""

    def __init__(self, lib, session, keys=None, tx_state=None, rx_state=None):
        cm = {s: k for s, k in (keys or {}).items() if not k.get("gcm")}
        super().__init__(lib, session, cm, tx_state, rx_state)
        for d in ("tx", "rx"):
            ss = sorted(s for s, k in (keys or {}).items() if k.get("gcm") and k.get(d) is not None)
            if ss:
                kw = dict(tx_index=[(tx_state or {}).get(s, 0) for s in ss]) if d == "tx" else dict(rx_index=[(rx_state or {}).get(s, -1) for s in ss])
                assert self.set_keys_gcm(ss, **{d: [keys[s][d] for s in ss]}, **kw) == 0

    def set_keys_gcm(self, streams, tx=None, rx=None, tx_index=None, rx_index=None):
        s = np.array(streams, np.int32)
        txa = None if tx is None else np.frombuffer(b"".join(tx), np.uint8)
        rxa = None if rx is None else np.frombuffer(b"".join(rx), np.uint8)
        ti = None if tx_index is None else np.array(tx_index, np.uint32)
        ri = None if rx_index is None else np.array(rx_index, np.int64)
        return self.lib.emu_gcm_srtcp_set_keys(self.h, p(s), len(streams), p(txa), p(rxa), p(ti), p(ri))


def rtcp_keys(rng, n, gcm, no_tx=(), no_rx=()):
    keys = CM.random_keys(rng, [s for s in range(n) if s not in gcm], no_tx, no_rx)
    for s in gcm:
        keys[s] = dict(tx=None if s in no_tx else G.random_master(rng), rx=None if s in no_rx else G.random_master(rng), gcm=True)
    return keys


def compound(rng, ssrc, n):
    """n >= 8 bytes that begin like a compound packet: a receiver report's header and SSRC (neither call looks behind them)"""
    return RC.write_rr(ssrc) + rng.integers(0, 256, n - 8, dtype=np.uint8).tobytes()


def laid_out_packets(rng, X, streams, sizes, trailer):
    """compound packets as build leaves them: 4-byte aligned, `trailer` zero bytes behind each -> (dgrams, wire, build count)"""
    wire, dg = bytearray(), []
    for s, n in zip(streams, sizes):
        dg.append((len(wire), n))
        wire += compound(rng, X.ssrc[s] if 0 <= s < X.n else 1, n) + bytes((trailer + 3) & ~3) if n else b""
    w = TC.aligned_bytes(len(wire) + 8)
    w[:len(wire)] = np.frombuffer(bytes(wire), np.uint8)
    return np.array(dg, np.int32).reshape(-1, 2), w, np.zeros(8, np.int32)


def test_host_srtcp_protect_against_the_model(host):
    n = 12
    rng = np.random.default_rng(311)
    X, _ = TC.sessions(n)
    gcm = (0, 1, 2, 3, 4, 5)
    keys = rtcp_keys(rng, n, gcm, no_tx=(5, 11))
    index = {0: 0, 1: 65535, 2: 65536, 3: 2 ** 31 - 1, 4: 2 ** 31, 6: 7, 7: 2 ** 31}
    ses = HostRtcpSes(host, X, keys, tx_state=index)
    tx_state = {s: index.get(s, 0) for s in range(n)}
    streams = list(range(n))
    sizes = [8, 12, 24, 40, 56, 20, 300, 52, 0, 28, 160, 20]
    for call in range(2):
        dg, wire, bc = laid_out_packets(rng, X, streams, sizes, 20)
        plain_dg, plain = dg.copy(), wire.copy()
        want = G.model_protect_rtcp(keys, tx_state, n, streams, False, dg, wire)
        r, got = ses.protect(streams, bc, dg, wire, trailer=20)
        assert r == 0 and got == want["count"], (got, want["count"])
        assert np.array_equal(dg, want["dgrams"]) and np.array_equal(wire, want["wire"])
        tx_state = want["tx_state"]
        assert ses.index() == ([tx_state[s] for s in range(n)], [-1] * n)
        if call == 0:
            assert got == dict(TC.count_dict([0] * 8), ok=7, skipped=1, no_key=2, exhausted=2)
            for s in (0, 1, 2, 3):                                     # GCM: the word is the LAST four bytes, the tag in front of it
                off, ln = (int(v) for v in dg[s])
                assert ln == sizes[s] + 20 and int.from_bytes(wire[off + ln - 4:off + ln].tobytes(), "big") == 0x80000000 | index[s]
                assert np.array_equal(wire[off:off + 8], plain[off:off + 8])
            off, ln = (int(v) for v in dg[6])                           # HMAC: the word in front of the tag
            assert ln == sizes[6] + 14 and int.from_bytes(wire[off + ln - 14:off + ln - 10].tobytes(), "big") == 0x80000000 | index[6]
        else:
            assert got["exhausted"] == 3 and got["ok"] == 6            # stream 3 has used its last index
    # the trailer: 20 while the session holds a GCM tx key; a room that ends before the 20 bytes; a refused list
    dg, wire, bc = laid_out_packets(rng, X, streams, sizes, 20)
    before = ses.snapshot()
    for t in (14, 16, 19):
        assert ses.protect(streams, bc, dg, wire, trailer=t)[0] == -1
    end = int(dg[1].sum())
    dg2, w2 = dg.copy(), wire.copy()
    want = G.model_protect_rtcp(keys, tx_state, n, streams[:2], False, dg2[:2].copy(), w2, wire_bytes=end + 19)
    r, got = ses.protect(streams[:2], bc, dg2[:2], w2, wire_bytes=end + 19, trailer=20)
    assert r == 0 and got == want["count"] and got["malformed"] == 1 and got["ok"] == 1 and np.array_equal(w2, want["wire"]) and dg2[1].tolist() == [0, 0]
    tx_state = want["tx_state"]
    bc[0] = -1
    snap = ses.snapshot()
    dg3, w3 = dg.copy(), wire.copy()
    r, got = ses.protect(streams, bc, dg3, w3, trailer=20)
    assert r == 0 and got == dict(TC.count_dict([0] * 8), ok=-1) and np.array_equal(dg3, dg) and np.array_equal(w3, wire) and ses.snapshot() == snap
    # without a GCM tx key the call takes 14 again
    assert ses.clear_keys(list(gcm)) == 0 and ses.protect(streams, np.zeros(8, np.int32), dg, wire, trailer=14)[0] == 0 and before != ses.snapshot()
    ses.close()


def receive_case(rng, n=12):
    """streams 0 .. 5 GCM, 6 .. 11 HMAC; 4 without an rx key, 10 not bound"""
    _, Y = TC.sessions(n)
    Y.bound[10] = 0
    keys = rtcp_keys(rng, n, (0, 1, 2, 3, 4, 5), no_rx=(4,))
    rx_state = {s: -1 for s in range(n)}
    rx_state.update({2: 1000, 3: 2 ** 31 - 2, 7: 500})
    k2, ssrc = G.session_keys(keys[2]["rx"], 3), Y.ssrc[2]
    idx = iter(range(1001, 1100))

    def flip(d, at, bit=0x10):
        return d[:at] + bytes([d[at] ^ bit]) + d[at + 1:]
    items = [("len_%d" % m, G.protect_rtcp_packet(k2, compound(rng, ssrc, m), next(idx)), "ok") for m in (8, 12, 24, 40, 56, 300)]
    items += [("odd_%d" % m, G.protect_rtcp_packet(k2, compound(rng, ssrc, 40)[:m], next(idx)), "ok") for m in (9, 27, 38)]
    items.append(("e0", G.protect_rtcp_packet(k2, compound(rng, ssrc, 40), next(idx), e=0), "ok"))
    items.append(("e0_odd", G.protect_rtcp_packet(k2, compound(rng, ssrc, 40)[:29], next(idx), e=0), "ok"))
    d = G.protect_rtcp_packet(k2, compound(rng, ssrc, 56), next(idx))
    items += [("copy_a", d, "ok"), ("copy_b", d, "ok")]
    d = G.protect_rtcp_packet(k2, compound(rng, ssrc, 56), next(idx))
    items += [("flip_tag", flip(d, len(d) - 5), "auth_failed"), ("flip_tag_first", flip(d, len(d) - 20), "auth_failed"), ("flip_index", flip(d, len(d) - 3, 0x01), "auth_failed"),
              ("flip_e", flip(d, len(d) - 4, 0x80), "auth_failed"), ("flip_body", flip(d, 20), "auth_failed"), ("flip_header", flip(d, 1), "auth_failed"),
              ("one_byte_cut", d[:-1], "auth_failed"), ("wrong_key", G.protect_rtcp_packet(G.session_keys(bytes(28), 3), d[:40], next(idx)), "auth_failed"),
              ("hmac_layout", CM.protect_packet(CM.session_keys(bytes(30)), d[:40], 0), "auth_failed"),
              ("equal_to_record", G.protect_rtcp_packet(k2, compound(rng, ssrc, 24), 1000), "replayed"),
              ("replayed_and_forged", flip(G.protect_rtcp_packet(k2, compound(rng, ssrc, 24), 3), 9), "replayed"),
              ("len_27", d[:8] + d[-19:], "malformed"), ("len_22", d[:22], "malformed"), ("len_21", d[:21], "malformed"),
              ("len_28_empty", G.protect_rtcp_packet(k2, compound(rng, ssrc, 8), next(idx)), "ok")]
    for s, index in ((0, 0), (1, 2 ** 31 - 1), (3, 2 ** 31 - 1), (5, 77)):
        items.append(("stream_%d" % s, G.protect_rtcp_packet(G.session_keys(keys[s]["rx"], 3), compound(rng, Y.ssrc[s], 28), index), "ok"))
    items.append(("record_at_the_end", G.protect_rtcp_packet(G.session_keys(keys[3]["rx"], 3), compound(rng, Y.ssrc[3], 28), 2 ** 31 - 2), "replayed"))
    items.append(("no_key", G.protect_rtcp_packet(G.session_keys(bytes(28), 3), compound(rng, Y.ssrc[4], 28), 3), "no_key"))
    items.append(("no_key_short", G.protect_rtcp_packet(G.session_keys(bytes(28), 3), compound(rng, Y.ssrc[4], 28), 3)[:23], "no_key"))
    items.append(("unbound", G.protect_rtcp_packet(k2, compound(rng, Y.ssrc[10], 28), 3), "unknown_ssrc"))
    for s, index, v in ((6, 0, "ok"), (7, 501, "ok"), (7, 500, "replayed"), (9, 65536, "ok")):       # the HMAC streams beside them
        items.append(("hmac_%d_%d" % (s, index), CM.protect_packet(CM.session_keys(keys[s]["rx"]), compound(rng, Y.ssrc[s], 40), index), v))
    items.append(("gcm_on_hmac_stream", G.protect_rtcp_packet(k2, compound(rng, Y.ssrc[8], 40), 9), "auth_failed"))
    order = rng.permutation(len(items))
    return Y, keys, rx_state, [items[i] for i in order]


@pytest.mark.parametrize("align", [0, 1, 2, 3])
def test_host_srtcp_unprotect_against_the_model(host, align):
    rng = np.random.default_rng(421)
    Y, keys, rx_state, items = receive_case(rng)
    dg, wire = CM.lay_out(rng, [k[1] for k in items], align=[align])
    assert all(int(o) % 4 == align for o in dg[:, 0])
    dg = np.concatenate([dg, np.array([[wire.size - 10, 40], [-4, 30], [wire.size, 28]], np.int32)])
    want = G.model_unprotect_rtcp(Y, keys, rx_state, dg, wire)
    assert want["verdicts"][:len(items)] == [k[2] for k in items], [(k[0], k[2], v) for k, v in zip(items, want["verdicts"]) if k[2] != v]
    assert set(want["verdicts"]) == {"ok", "malformed", "unknown_ssrc", "no_key", "auth_failed", "replayed"}
    ses = HostRtcpSes(host, Y, keys, rx_state=rx_state)
    w = wire.copy()
    out, cnt = ses.unprotect(dg, w)
    assert cnt == want["count"], (cnt, want["count"])
    assert np.array_equal(out, want["dgrams"]) and np.array_equal(w, want["wire"])
    for (off, ln), v in zip(dg.tolist()[:len(items)], want["verdicts"]):                      # a rejected datagram keeps every byte
        assert v == "ok" or np.array_equal(w[off:off + ln], wire[off:off + ln])
    assert ses.index()[1] == [want["rx_state"][s] for s in range(Y.n)]
    # the same call again: what was accepted is now replayed, every byte kept
    w2 = w.copy()
    out2, cnt2 = ses.unprotect(dg, w2)
    want2 = G.model_unprotect_rtcp(Y, keys, want["rx_state"], dg, w)
    assert cnt2 == want2["count"] and cnt2["ok"] == 0 and cnt2["replayed"] >= cnt["ok"] and not out2.any() and np.array_equal(w2, w)
    ses.close()


def test_host_srtcp_published_and_fixture_datagrams(host, fixture):
    cases = [(RFC_KEYS["ke"], RFC_KEYS["ks"], (0x4d617273, 0x5d4, 1), RFC_RTCP, RFC_SRTCP)] + fixture["srtcp"]      # (section 16.2.2 has the same SSRC: on its own below)
    n = len(cases)
    X = RC.Session([int(c[2][0]) for c in cases], [0] * n, packet_samples=640)
    rng = np.random.default_rng(9)
    ses = HostRtcpSes(host, X)
    for s, c in enumerate(cases):
        assert host.emu_gcm_srtcp_set_session(ses.h, s, 1, p(buf(c[0])), p(buf(c[1])), -1) == 0
        assert host.emu_gcm_srtcp_set_session(ses.h, s, 0, p(buf(c[0])), p(buf(c[1])), int(c[2][1])) == 0
    live = list(range(n))
    dg, wire = CM.lay_out(rng, [cases[s][4] for s in live])
    out, cnt = ses.unprotect(dg, wire)
    assert cnt == dict(TC.count_dict([0] * 8), ok=len(live))
    for (off, ln), s in zip(out.tolist(), live):
        assert wire[off:off + ln].tobytes() == cases[s][3]
    assert [ses.index()[1][s] for s in live] == [int(cases[s][2][1]) for s in live]
    # protect writes E = 1 only: the packets of a multiple of 4 bytes come out as libcrypto made them
    sel = [s for s in live if cases[s][2][2] == 1 and len(cases[s][3]) % 4 == 0]
    dg, wire = CM.lay_out(rng, [cases[s][3] + bytes(20) for s in sel], align=[0])
    dg[:, 1] -= 20
    r, got = ses.protect(sel, np.zeros(8, np.int32), dg, wire, trailer=20)
    assert r == 0 and got == dict(TC.count_dict([0] * 8), ok=len(sel)) and 0 in sel and len(sel) >= 5
    for (off, ln), s in zip(dg.tolist(), sel):
        assert wire[off:off + ln].tobytes() == cases[s][4], s
    ses.close()
    # section 16.2.2: E = 0, accepted on receipt
    X = RC.Session([0x4d617273], [0], packet_samples=640)
    ses = HostRtcpSes(host, X)
    assert host.emu_gcm_srtcp_set_session(ses.h, 0, 1, p(buf(RFC_KEYS["ke"])), p(buf(RFC_KEYS["ks"])), 0x5d3) == 0
    dg, wire = CM.lay_out(rng, [RFC_SRTCP_E0])
    out, cnt = ses.unprotect(dg, wire)
    assert cnt["ok"] == 1 and wire[out[0, 0]:out[0, 0] + out[0, 1]].tobytes() == RFC_RTCP and ses.index()[1] == [0x5d4]
    ses.close()


def test_a_call_without_the_gcm_kernel_fails_closed(host):
    """A call issued -- a graph captured -- before the session's first GCM key holds only the older kernel.  The older pass alone, as such a
    graph replays it, must let nothing of a GCM-keyed stream out in the clear and nothing unauthenticated in: no_key, voided, untouched"""
    rng = np.random.default_rng(5)
    ses = mixed_session(rng, 0)
    h = HostGcm(host, ses)
    rec = np.array([[0, 10, 0, 0, 40], [2, 10, 0, 40, 40], [1, 11, 1, 80, 33]], np.int32)
    dg, wire, c = h.pack(rec, 3, rng.integers(0, 256, 200, dtype=np.uint8))
    packed, sc, cnt = wire.copy(), np.array([3] + [0] * 7, np.int32), np.full(8, -9, np.int32)
    host.alone["srtp_protect"](h.h, p(rec), p(sc), 3, p(dg), p(wire), wire.size, p(cnt))
    assert TS.count_dict(cnt) == dict(TS.count_dict([0] * 8), ok=1, no_key=2) and dg[0].tolist() == [0, 0] == dg[2].tolist() and dg[1, 1] == 12 + 40 + 10
    rx = HostGcm(host, G.loop_session(ses))
    keys = G.session_keys(ses["srtp"][0]["tx"])
    d = G.protect_packet(keys, R.build(ses["streams"][0]["ssrc"], 96, 7, 0, b"q" * 30), 0)
    for alias in (False, True):
        dgi, w = TS.lay_out(rng, [d])
        before, out = w.copy(), dgi if alias else np.full((1, 2), -7, np.int32)
        host.alone["srtp_unprotect"](rx.h, p(dgi), 1, p(w), w.size, p(out), p(cnt))
        assert TS.count_dict(cnt) == dict(TS.count_dict([0] * 8), no_key=1) and out.tolist() == [[0, 0]] and np.array_equal(w, before) and rx.rx_index([0]) == [-1]
    h.close()
    rx.close()
    # SRTCP likewise
    X, _ = TC.sessions(4)
    keys = rtcp_keys(rng, 4, (0, 1))
    s = HostRtcpSes(host, X, keys, rx_state={0: 5})
    dg, wire, bc = laid_out_packets(rng, X, [0, 2], [24, 24], 20)
    plain, cnt = wire.copy(), np.full(12, -9, np.int32)
    idx = np.array([0, 2], np.int32)
    assert host.alone["srtcp_protect"](s.h, 4, 20, p(idx), 2, p(bc), p(dg), p(wire), wire.size, p(cnt)) == 0
    assert TC.count_dict(cnt[:8]) == dict(TC.count_dict([0] * 8), ok=1, no_key=1) and dg[0].tolist() == [0, 0] and np.array_equal(wire[:24], plain[:24])
    assert s.index([0])[0] == [0]
    d = G.protect_rtcp_packet(G.session_keys(keys[0]["rx"], 3), compound(rng, X.ssrc[0], 24), 9)
    for alias in (False, True):
        dgi, w = CM.lay_out(rng, [d])
        before, out = w.copy(), dgi if alias else np.full((1, 2), -7, np.int32)
        assert host.alone["srtcp_unprotect"](s.h, p(dgi), 1, p(w), w.size, p(out), p(cnt)) == 0
        assert TC.count_dict(cnt[:8]) == dict(TC.count_dict([0] * 8), no_key=1) and out.tolist() == [[0, 0]] and np.array_equal(w, before) and s.index([0])[1] == [5]
    s.close()


# ---- the control plane ------------------------------------------------------------------------------------------------------------------------------------
def test_control_plane(host):
    rng = np.random.default_rng(77)
    ses = R.random_session(rng, 5, 640, 0, unbound=(4,))
    ses["srtp"] = {}
    h = HostGcm(host, ses)
    key = [G.random_master(rng) for _ in range(5)]
    old = [rng.integers(0, 256, 30, dtype=np.uint8).tobytes() for _ in range(2)]

    def mirror():
        return [(host.emu_srtp_mirror(h.h, s, 0), host.emu_srtp_mirror(h.h, s, 1)) for s in range(5)]
    # a tx key needs a trailer of 16; an rx key does not
    assert h.set_keys([0], 16, tx=key[:1]) == -1 and h.set_trailer(15) == 0 and h.set_keys([0], 16, tx=key[:1]) == -1 and host.emu_gcm_srtp_any(h.h, 0) == 0
    assert h.set_keys([1], 16, rx=key[1:2]) == 0 and mirror()[1] == (0, 16) and host.emu_gcm_srtp_any(h.h, 1) == 1 and host.emu_gcm_srtp_any(h.h, 0) == 0
    assert h.set_trailer(16) == 0 and h.set_keys([0], 16, tx=key[:1]) == 0 and mirror()[0] == (16, 0)
    # the trailer never goes below a keyed sender's tag, which is now 16
    for t in (10, 15, 0, 17, -1):
        assert h.set_trailer(t) == -1
    # refusals: nothing changes.  (A 27-byte master cannot be seen by the C call, whose arrays carry no length: the binding refuses it.)
    for streams, kw in (([5], dict(tx=key[:1])), ([-1], dict(tx=key[:1])), ([1, 1], dict(tx=key[:2])), ([], dict(tx=[])), ([1], dict())):
        m, words = mirror(), [host.emu_srtp_key_words(h.h, s) for s in range(5)]
        assert h.set_keys(streams, 16, **kw) == -1 and m == mirror() and words == [host.emu_srtp_key_words(h.h, s) for s in range(5)]
    assert h.set_keys([1], 16, rx=key[1:2]) == 0 and h.set_keys([1], 8, rx=old[:1]) == -1       # solo_srtp_set_keys keeps refusing every tag but 4 and 10
    # one key per stream and direction: the last set call wins, whichever transform it names
    rec = np.zeros(64, np.uint32)
    assert h.set_keys([0], 10, tx=old[:1]) == 0 and mirror()[0] == (10, 0) and host.emu_gcm_srtp_any(h.h, 0) == 0
    host.emu_gcm_srtp_record(h.h, 0, 0, p(rec))
    assert rec[58:61].tolist() == [10, 1, 0] and h.set_trailer(10) == 0 and h.set_keys([0], 16, tx=key[:1]) == -1 and h.set_trailer(16) == 0
    assert h.set_keys([0], 16, tx=key[:1]) == 0 and mirror()[0] == (16, 0)
    host.emu_gcm_srtp_record(h.h, 0, 0, p(rec))
    assert rec[58:61].tolist() == [16, 1, 1] and not rec[52:58].any()
    # clear_keys and unbind keep their meaning
    assert h.clear_keys([0]) == 0 and host.emu_srtp_key_words(h.h, 0) == 0 and mirror()[0] == (0, 0) and h.set_trailer(0) == 0
    assert host.emu_srtp_key_words(h.h, 1) > 50 and h.unbind([1]) == 0 and host.emu_srtp_key_words(h.h, 1) == 0 and mirror()[1] == (0, 0) and host.emu_gcm_srtp_any(h.h, 1) == 0
    h.close()
    # SRTCP
    X, _ = TC.sessions(4)
    s = HostRtcpSes(host, X)
    assert s.index() == ([0] * 4, [-1] * 4)
    for streams, kw in (([4], dict(tx=key[:1])), ([1, 1], dict(tx=key[:2])), ([], dict(tx=[])), ([1], dict()), ([1], dict(tx=key[:1], tx_index=[2 ** 31 + 1])),
                        ([1], dict(rx=key[:1], rx_index=[-2])), ([1], dict(rx=key[:1], rx_index=[2 ** 31]))):
        before = s.snapshot()
        assert s.set_keys_gcm(streams, **kw) == -1 and s.snapshot() == before
    assert s.set_keys_gcm([1, 2], tx=key[:2], tx_index=[7, 8]) == 0 and s.set_keys_gcm([1], rx=key[2:3], rx_index=[40]) == 0 and s.index([1, 2]) == ([7, 8], [40, -1])
    assert [host.emu_gcm_srtcp_mirror(s.h, 1, d) for d in (0, 1)] == [2, 2] and [host.emu_gcm_srtcp_mirror(s.h, 2, d) for d in (0, 1)] == [2, 0]
    host.emu_gcm_srtcp_record(s.h, 1, 0, p(rec))
    assert rec[58:61].tolist() == [16, 1, 1]
    assert s.set_keys([1], tx=[bytes(30)]) == 0 and host.emu_gcm_srtcp_mirror(s.h, 1, 0) == 1 and s.index([1]) == ([0], [40])     # the last set call wins
    assert s.clear_keys([1, 2]) == 0 and host.emu_srtcp_key_words(s.h, 1) == 0 and host.emu_srtcp_key_words(s.h, 2) == 0 and s.index([1, 2]) == ([0, 0], [-1, -1])
    assert [host.emu_gcm_srtcp_mirror(s.h, k, 0) for k in (1, 2)] == [0, 0]
    assert [host.emu_srtcp_trailer_ok(t) for t in (-1, 0, 14, 16, 17, 18, 19, 20, 21, 24)] == [-1, 0, 0, 0, -1, -1, -1, 0, -1, -1]
    s.close()


# ---- the binding, the ABI, the kernels ----------------------------------------------------------------------------------------------------------------------
def test_binding_checks():
    import solo_amd
    torch = pytest.importorskip("torch")
    o = object.__new__(solo_amd.Rtp)
    o.n_rows = o.n_streams = 8
    o.packet_samples, o.level_id, o.trailer = 640, 0, 15
    o.torch, o.lib, o.h, o.device = torch, T.NoLib(), None, torch.device("cpu")
    o._stream = lambda: None
    k = bytes(28)
    for kw in (dict(streams=[0, 0], rx=[k, k]), dict(streams=[8], rx=[k]), dict(streams=[0], rx=[k[:27]]), dict(streams=[0], rx=[bytes(30)]), dict(streams=[0]),
               dict(streams=[0, 1], rx=[k]), dict(streams=[0], tx=[k]), dict(streams=[0], rx=[k], rx_roc=2 ** 32), dict(streams=[0], rx=[k], rx_roc=[1, 2])):
        with pytest.raises(ValueError):
            o.set_keys_gcm(**kw)
    for kw in (dict(streams=[0, 0], tx=[k, k]), dict(streams=[8], tx=[k]), dict(streams=[0], tx=[k[:27]]), dict(streams=[0], tx=[bytes(30)]), dict(streams=[0]),
               dict(streams=[0], tx=[k], tx_index=2 ** 31 + 1), dict(streams=[0], rx=[k], rx_index=-2), dict(streams=[0], rx=[k], rx_index=2 ** 31)):
        with pytest.raises(ValueError):
            o.set_rtcp_keys_gcm(**kw)
    with pytest.raises(ValueError):
        o.set_keys(streams=[0], rx=[bytes(30)], tag_bytes=16)          # 16 is not a tag of the older transform
    c = object.__new__(solo_amd.Rtcp)
    c.n_rows = c.n_streams = 8
    c.trailer, c.torch, c.lib, c.h, c.device = 16, torch, T.NoLib(), 1, torch.device("cpu")
    c._stream = lambda: None
    for bad in (-1, 17, 18, 19, 21, "x"):
        with pytest.raises(ValueError):
            c.set_trailer(bad)
    # protect_rtcp: the library alone knows the session's keys; its -1 under a trailer below 20 is the GCM rule, and a ValueError
    class Dev(T.FakeDev):
        device = torch.device("cpu")

        def data_ptr(self):
            return 64

    class Lib:
        def __init__(self, r):
            self.r = r

        def solo_srtcp_protect(self, *a):
            return self.r
    I32, U8 = torch.int32, torch.uint8
    good = dict(rtcp=c, streams=Dev((5,), I32), build_count=Dev((8,), I32), dgrams=Dev((5, 2), I32), wire=Dev((999,), U8))
    o.lib = Lib(-1)
    with pytest.raises(ValueError, match="20"):
        o.protect_rtcp(**good)
    c.trailer = 20
    with pytest.raises(RuntimeError):                                  # with the longer trailer a -1 is not that rule
        o.protect_rtcp(**good)
    o.lib, c.trailer = Lib(0), 16
    assert o.protect_rtcp(**good).shape == (8,)
    assert not hasattr(o, "_gcm_rtcp_tx") and not any("gcm" in k for k in vars(o))       # the binding keeps no mirror of its own
    c.h = None
    assert solo_amd.SRTP_GCM_MASTER_BYTES == 28 and solo_amd.SRTCP_GCM_TRAILER_BYTES == 20 and solo_amd.SRTP_GCM_TAG_BYTES == 16


def test_symbols_declared_exported_listed_and_bound(host):
    import solo_amd
    hdr = T.header_text()
    lib = T.built_library()
    bound = solo_amd.load_library()
    for name, n_args in (("solo_srtp_set_keys_gcm", 7), ("solo_srtcp_set_keys_gcm", 8)):
        assert name in solo_amd.ABI_SYMBOLS and (name + "(") in hdr.replace(" (", "("), name
        assert hasattr(lib, name), name
        assert len(getattr(bound, name).argtypes) == n_args and getattr(bound, name).restype is C.c_int32, name
    for d in ("SOLO_SRTP_GCM_MASTER_BYTES 28", "SOLO_SRTP_GCM_TAG_BYTES 16", "SOLO_SRTCP_GCM_TRAILER_BYTES 20", "SOLO_SRTP_MASTER_BYTES 30", "SOLO_SRTCP_TRAILER_BYTES 14"):
        assert "#define " + d in hdr, d
    assert host.emu_srtp_sizes(1) == 256 and [host.emu_srtcp_sizes(k) for k in range(1, 6)] == [256, 16, 4, 14, 532]      # the records keep their sizes
    assert len(bound.solo_srtp_protect.argtypes) == 9 and len(bound.solo_srtcp_protect.argtypes) == 10 and len(bound.solo_srtp_set_keys.argtypes) == 8
    for m in ("set_keys_gcm", "set_rtcp_keys_gcm"):
        assert callable(getattr(solo_amd.Rtp, m)), m
    src = open(os.path.join(T.ROOT, "solo_amd", "csrc", "solo_srtp_gcm.h")).read()
    srtp = open(os.path.join(T.ROOT, "solo_amd", "csrc", "solo_srtp.h")).read()
    for name in ("sx_aes_block", "sx_srtp_guess_index", "sx_srtp_rx_fold"):                       # used, not copied
        assert len(re.findall(r"SX_HD \w+ %s\(" % name, srtp)) == 1 and not re.search(r"SX_HD \w+ %s\(" % name, src) and name + "(" in src, name
    assert "sx_rtp_header_walk(" in src and "sx_rtp_be32(" in src and '#include "solo_srtp_gcm.h"' in open(os.path.join(T.ROOT, "solo_amd", "csrc", "solo_api.hip")).read()


def test_capture_claims_name_a_test():
    """the header's GCM block names the tests of tests/test_gpu_srtp_gcm.py that capture the four device calls with GCM keys"""
    import ast
    import test_gpu_srtp_gcm as GPU
    text = open(os.path.join(T.ROOT, "include", "solo_mi355x.h")).read()
    m = re.search(r"/\* AEAD_AES_128_GCM \(RFC 7714\).*?\*/", text, flags=re.S)
    tests = {x.name for x in ast.parse(open(GPU.__file__).read()).body if isinstance(x, ast.FunctionDef) and x.name.startswith("test_")}
    assert m and set(GPU.CAPTURED) == {"solo_srtp_protect", "solo_srtp_unprotect", "solo_srtcp_protect", "solo_srtcp_unprotect"} and set(GPU.CAPTURED.values()) <= tests
    for name in GPU.CAPTURED.values():
        assert "tests/test_gpu_srtp_gcm.py" in m.group(0) and name in m.group(0), name


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="no LLVM binutils on this box")
def test_gcm_kernels_use_no_scratch():
    import solo_amd
    T.built_library()
    sys.path.insert(0, os.path.join(T.ROOT, "tools"))
    from kernel_resources import kernel_resources
    seen = kernel_resources(solo_amd.LIB_PATH)
    for frag in KERNELS + OLD_KERNELS:
        hits = [r for name, r in seen.items() if frag in name]
        assert len(hits) == 1, (frag, len(hits))
        assert hits[0]["scratch"] == 0, (frag, hits[0])
    for frag in KERNELS:                                               # 64 lanes of 256-byte tables and the AES table: under 20 KB a workgroup
        assert 16384 < [r for name, r in seen.items() if frag in name][0]["lds"] <= 20480


# ---- the same source as a stand-alone program under the sanitisers -------------------------------------------------------------------------------------------
def test_stand_alone_build_under_the_sanitisers(tmp_path):
    """tests/srtp_gcm_host.cpp with its own main, -fsanitize=address,undefined: the hostile families of both stages in through a file, in
    heap blocks of exactly their size, every output back through a file and against the model; any report of a sanitiser ends the
    program with a non-zero status"""
    exe = str(tmp_path / "srtp_gcm_asan")
    flags = [f for f in FLAGS if f not in ("-shared", "-fPIC", "-O2")] + ["-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                                                         "-DSRTP_GCM_MAIN"]
    cxx = os.environ.get("CXX", "g++")
    if os.path.basename(cxx).startswith("g++"):                       # the runtimes inside the program: nothing has to load ahead of it
        flags += ["-static-libasan", "-static-libubsan"]
    subprocess.check_call([cxx] + flags + [source("srtp_gcm"), "-o", exe])

    def run(name, stage, n_streams, ssrc, start, masters, dg, wire):
        fin, fout = str(tmp_path / (name + ".in")), str(tmp_path / (name + ".out"))
        with open(fin, "wb") as f:
            f.write(np.array([n_streams, dg.shape[0], wire.size, stage, 0, 0, 0, 0], np.int32).tobytes())
            f.write(np.array(ssrc, np.uint32).tobytes() + np.array(start, np.int64).tobytes() + b"".join(masters) + dg.tobytes() + wire.tobytes())
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        raw, n = open(fout, "rb").read(), dg.shape[0]
        return (np.frombuffer(raw[:8 * n], np.int32).reshape(n, 2), np.frombuffer(raw[8 * n:8 * n + 32], np.int32),
                np.frombuffer(raw[8 * n + 32:8 * n + 32 + 8 * n_streams], np.int64), np.frombuffer(raw[8 * n + 32 + 8 * n_streams:], np.uint8))
    rng = np.random.default_rng(516)
    ses = R.random_session(rng, 6, 640, 5)
    ses["srtp"] = {s: G.gcm_entry(rng) for s in range(6)}
    roc0 = {s: 7 * s for s in range(6)}
    state = S.new_state(ses, roc0)
    kinds = G.hostile_set(ses, state, 2, rng, R) + G.hostile_set(ses, state, 5, rng, R)
    dg, wire = TS.lay_out(rng, [k[1] for k in kinds], front=0, gap=0)
    wire = wire[:int(dg[-1].sum())]                                   # the last datagram ends with the block
    dg = np.concatenate([dg, np.array([[wire.size - 10, 40], [-4, 30], [wire.size, 16]], np.int32)])
    want = G.model_unprotect(ses, state, dg, wire)
    assert want["verdicts"][:len(kinds)] == [k[2] for k in kinds]
    out, cnt, index, w = run("srtp", 0, 6, [ses["streams"][s]["ssrc"] for s in range(6)], [roc0[s] for s in range(6)], [ses["srtp"][s]["rx"] for s in range(6)], dg, wire)
    assert TS.count_dict(cnt) == want["count"] and np.array_equal(out, want["dgrams"]) and np.array_equal(w, want["wire"])
    assert index.tolist() == [want["state"][s]["index"] for s in range(6)]
    # SRTCP: every stream of the case under a GCM rx key (the program keys them all)
    Y, keys, rx_state, items = receive_case(rng)
    for s in range(Y.n):
        if not keys[s].get("gcm") or keys[s].get("rx") is None:
            keys[s] = dict(tx=None, rx=G.random_master(rng), gcm=True)
    Y.bound[10] = 1
    dg, wire = CM.lay_out(rng, [k[1] for k in items], front=0, gap=0)
    wire = wire[:int(dg[-1].sum())]
    dg = np.concatenate([dg, np.array([[wire.size - 10, 40], [-4, 30], [wire.size, 28]], np.int32)])
    want = G.model_unprotect_rtcp(Y, keys, rx_state, dg, wire)
    assert {"ok", "malformed", "auth_failed", "replayed"} <= set(want["verdicts"])
    out, cnt, index, w = run("srtcp", 1, Y.n, list(Y.ssrc), [rx_state[s] for s in range(Y.n)], [keys[s]["rx"] for s in range(Y.n)], dg, wire)
    assert TC.count_dict(cnt) == want["count"] and np.array_equal(out, want["dgrams"]) and np.array_equal(w, want["wire"])
    assert index.tolist() == [want["rx_state"][s] for s in range(Y.n)]

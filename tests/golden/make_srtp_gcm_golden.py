"""Writes tests/golden/srtp_gcm_cases.npz: AEAD_AES_128_GCM answers made by the system's libcrypto (EVP_aes_128_gcm through ctypes), the
yardstick that nobody here wrote.  Run from the repository root:  python tests/golden/make_srtp_gcm_golden.py

  cases     (key, iv, aad, plaintext) -> (ciphertext, tag) for every pair of an AAD length of AAD_LENGTHS and a plaintext length of
            PT_LENGTHS, three random keys each; the byte strings lie back to back in *_blob, case i at its offset
  srtp      whole SRTP datagrams (RFC 7714 section 9): RTP packets of tests/rtp_model.py under random SESSION keys and salts, the IV and
            the associated data assembled here, the AEAD done by libcrypto
  srtcp     whole SRTCP datagrams (section 10) likewise, with E = 1 and E = 0
tests/test_srtp_gcm_model.py imports gcm() from here for fresh random cases where libcrypto loads."""
import ctypes as C
import ctypes.util
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
AAD_LENGTHS = [0, 8, 12, 16, 20, 28, 40]
PT_LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 300]
EVP_CTRL_GCM_SET_IVLEN, EVP_CTRL_GCM_GET_TAG = 0x9, 0x10
_lib = None


def libcrypto():
    """the machine's libcrypto, or None"""
    global _lib
    if _lib is None:
        name = ctypes.util.find_library("crypto")
        try:
            lib = C.CDLL(name) if name else None
            if lib is not None:
                lib.EVP_CIPHER_CTX_new.restype = C.c_void_p
                lib.EVP_aes_128_gcm.restype = C.c_void_p
                lib.EVP_CIPHER_CTX_free.argtypes = [C.c_void_p]
                lib.EVP_EncryptInit_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_char_p]
                lib.EVP_EncryptUpdate.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int), C.c_char_p, C.c_int]
                lib.EVP_EncryptFinal_ex.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int)]
                lib.EVP_CIPHER_CTX_ctrl.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
            _lib = lib or False
        except (OSError, AttributeError):
            _lib = False
    return _lib or None


def gcm(key, iv, aad, pt):
    """AES-128-GCM with a 12-byte IV by libcrypto -> (ciphertext, 16-byte tag)"""
    lib = libcrypto()
    ctx = lib.EVP_CIPHER_CTX_new()
    try:
        n = C.c_int(0)
        assert lib.EVP_EncryptInit_ex(ctx, lib.EVP_aes_128_gcm(), None, None, None) == 1
        assert lib.EVP_CIPHER_CTX_ctrl(ctx, EVP_CTRL_GCM_SET_IVLEN, len(iv), None) == 1
        assert lib.EVP_EncryptInit_ex(ctx, None, None, bytes(key), bytes(iv)) == 1
        if aad:
            assert lib.EVP_EncryptUpdate(ctx, None, C.byref(n), bytes(aad), len(aad)) == 1
        out = C.create_string_buffer(len(pt) + 16)
        got = 0
        if pt:
            assert lib.EVP_EncryptUpdate(ctx, out, C.byref(n), bytes(pt), len(pt)) == 1
            got = n.value
        assert lib.EVP_EncryptFinal_ex(ctx, C.cast(C.byref(out, got), C.c_char_p), C.byref(n)) == 1
        got += n.value
        tag = C.create_string_buffer(16)
        assert lib.EVP_CIPHER_CTX_ctrl(ctx, EVP_CTRL_GCM_GET_TAG, 16, tag) == 1
        assert got == len(pt)
        return out.raw[:got], tag.raw
    finally:
        lib.EVP_CIPHER_CTX_free(ctx)


def blob(items):
    """[bytes] -> (uint8 blob, int32 offsets [n + 1])"""
    off = np.zeros(len(items) + 1, np.int32)
    off[1:] = np.cumsum([len(b) for b in items])
    return np.frombuffer(b"".join(items), np.uint8), off


def main():
    sys.path.insert(0, os.path.dirname(HERE))
    import rtp_model as R
    rng = np.random.default_rng(7714)

    def rnd(n):
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    out = {}
    keys, ivs, aads, pts, cts, tags = [], [], [], [], [], []
    for _ in range(3):
        for na in AAD_LENGTHS:
            for npt in PT_LENGTHS:
                k, iv, a, p = rnd(16), rnd(12), rnd(na), rnd(npt)
                c, t = gcm(k, iv, a, p)
                keys.append(k), ivs.append(iv), aads.append(a), pts.append(p), cts.append(c), tags.append(t)
    out["key"], out["iv"], out["tag"] = (np.frombuffer(b"".join(x), np.uint8).reshape(len(x), -1) for x in (keys, ivs, tags))
    for name, items in (("aad", aads), ("pt", pts), ("ct", cts)):
        out[name + "_blob"], out[name + "_off"] = blob(items)
    # SRTP: header 12, header 20 with the level extension, a CSRC header; sequence numbers on both sides of a rollover
    ke, ks, meta, plain, wire = [], [], [], [], []
    for i, (npt, kw) in enumerate([(n, kw) for kw in (dict(), dict(ext=R.level_ext(3, 0x2A)), dict(csrc=[11, 12])) for n in (0, 1, 16, 33, 160, 300)]):
        k, s = rnd(16), rnd(12)
        ssrc, roc, seq = int(rng.integers(1, 2 ** 32)), int(rng.integers(0, 2 ** 32)) if i % 3 else 0, (65534 + i) % 65536
        rtp = R.build(ssrc, 96, seq, int(rng.integers(0, 2 ** 32)), rnd(npt), **kw)
        hdr = len(rtp) - npt
        iv = bytes(a ^ b for a, b in zip(b"\0\0" + struct.pack(">IIH", ssrc, roc, seq), s))
        c, t = gcm(k, iv, rtp[:hdr], rtp[hdr:])
        ke.append(k), ks.append(s), meta.append((ssrc, roc, seq, hdr)), plain.append(rtp), wire.append(rtp[:hdr] + c + t)
    out["srtp_ke"], out["srtp_ks"] = (np.frombuffer(b"".join(x), np.uint8).reshape(len(x), -1) for x in (ke, ks))
    out["srtp_meta"] = np.array(meta, np.int64)              # ssrc, roc, seq, header bytes
    out["srtp_plain_blob"], out["srtp_plain_off"] = blob(plain)
    out["srtp_wire_blob"], out["srtp_wire_off"] = blob(wire)
    # SRTCP: compound packets of 8 .. 300 bytes (multiples of 4 and not: a receiver takes any length), E = 1 and E = 0
    ke, ks, meta, plain, wire = [], [], [], [], []
    for i, n in enumerate((8, 12, 24, 40, 56, 157, 300, 9, 24, 56)):
        k, s = rnd(16), rnd(12)
        ssrc, index, e = int(rng.integers(1, 2 ** 32)), int(rng.integers(0, 2 ** 31)), 0 if i >= 8 else 1
        pkt = struct.pack(">BBH", 0x80, 201, max(n // 4 - 1, 1)) + struct.pack(">I", ssrc) + rnd(n - 8)
        word = struct.pack(">I", (e << 31) | index)
        iv = bytes(a ^ b for a, b in zip(b"\0\0" + struct.pack(">IHI", ssrc, 0, index), s))
        if e:
            c, t = gcm(k, iv, pkt[:8] + word, pkt[8:])
            d = pkt[:8] + c + t + word
        else:
            d = pkt + gcm(k, iv, pkt + word, b"")[1] + word
        ke.append(k), ks.append(s), meta.append((ssrc, index, e)), plain.append(pkt), wire.append(d)
    out["srtcp_ke"], out["srtcp_ks"] = (np.frombuffer(b"".join(x), np.uint8).reshape(len(x), -1) for x in (ke, ks))
    out["srtcp_meta"] = np.array(meta, np.int64)             # ssrc, index, E
    out["srtcp_plain_blob"], out["srtcp_plain_off"] = blob(plain)
    out["srtcp_wire_blob"], out["srtcp_wire_off"] = blob(wire)
    path = os.path.join(HERE, "srtp_gcm_cases.npz")
    np.savez_compressed(path, **out)
    print("%s: %d cases, %d + %d datagrams, %d bytes" % (path, len(keys), len(out["srtp_meta"]), len(out["srtcp_meta"]), os.path.getsize(path)))


if __name__ == "__main__":
    main()

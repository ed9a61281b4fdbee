"""An independent model of AEAD_AES_128_GCM in the SRTP and the SRTCP stage (RFC 7714; include/solo_mi355x.h), written from the
specification's text -- not from the HIP source.  GHASH is SP 800-38D's algorithm on Python integers, bit by bit: a block is a 128-bit
integer whose most significant bit is the coefficient of x^0, and multiplying by x is a right shift with R = 0xE1 << 120 folded in.  AES,
the PRF of RFC 3711 section 4.3, the RTP header walk and the AES-CM / HMAC streams of a mixed session are those of tests/srtp_model.py
and tests/srtcp_model.py.

SRTP: a session is rtp_model's dict plus ses["srtp"] = {stream: entry}; an entry of srtp_model (tx / rx = 30-byte masters, tag 10 or 4) is
an AES-CM stream, an entry dict(tx=master28 or None, rx=master28 or None, tag=16, gcm=True) is a GCM stream; "tx_session" / "rx_session" =
dict(ke, ks) instead of a master is the test-only path for published session keys.
SRTCP: keys = {stream: dict(tx, rx)} as in srtcp_model, with gcm=True for a GCM stream."""
import functools
import struct

import numpy as np

import srtp_model as S
import srtcp_model as C

TAG = 16
MASTER = 28
RTCP_TRAILER = TAG + 4        # the tag, THEN the E || index word
R = 0xE1 << 120


# ---- GF(2^128) and GHASH (SP 800-38D sections 6.3, 6.4) -------------------------------------------------------------------------------------
def gf_mul(x, y):
    z, v = 0, y
    for i in range(127, -1, -1):              # bit 127 of the integer is x_0, the leftmost bit of the block
        if (x >> i) & 1:
            z ^= v
        v = (v >> 1) ^ R if v & 1 else v >> 1
    return z


def _blocks(b):
    b = b + bytes(-len(b) % 16)
    return [int.from_bytes(b[i:i + 16], "big") for i in range(0, len(b), 16)]


def ghash(h, a, c):
    """h: the hash key as 16 bytes -> 16 bytes"""
    hh, y = int.from_bytes(h, "big"), 0
    for x in _blocks(a) + _blocks(c) + [(8 * len(a)) << 64 | 8 * len(c)]:
        y = gf_mul(y ^ x, hh)
    return y.to_bytes(16, "big")


def _xor(a, b):
    return bytes(x ^ y for x, y in zip(a, b))


def gcm_encrypt(key, iv, aad, pt):
    """a 12-byte IV -> (ciphertext, 16-byte tag)"""
    assert len(iv) == 12
    ks = b"".join(S.aes_encrypt(key, iv + struct.pack(">I", j + 2)) for j in range((len(pt) + 15) // 16))
    ct = _xor(pt, ks)
    return ct, _xor(S.aes_encrypt(key, iv + b"\0\0\0\1"), ghash(S.aes_encrypt(key, bytes(16)), aad, ct))


def gcm_decrypt(key, iv, aad, ct, tag):
    """-> the plaintext, or None where the tag does not fit"""
    if _xor(S.aes_encrypt(key, iv + b"\0\0\0\1"), ghash(S.aes_encrypt(key, bytes(16)), aad, ct)) != bytes(tag):
        return None
    return gcm_encrypt(key, iv, b"", ct)[0]


# ---- keys -------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1024)
def session_keys(master28, label=0):
    """RFC 7714 section 11: the PRF of RFC 3711 with the 12-byte master salt padded on the right to 14; label 0 SRTP, 3 SRTCP"""
    mk, ms = bytes(master28[:16]), bytes(master28[16:28]) + b"\0\0"
    return dict(ke=S.derive(mk, ms, label, 16), ks=S.derive(mk, ms, label + 2, 14)[:12])


def _keys_of(entry, d, label=0):
    ses_keys = entry.get(d + "_session")
    return ses_keys if ses_keys is not None else session_keys(entry[d], label)


def _has(entry, d):
    return bool(entry) and (entry.get(d) is not None or entry.get(d + "_session") is not None)


# ---- SRTP, one packet ----------------------------------------------------------------------------------------------------------------------------
def rtp_iv(ks, ssrc, roc, seq):
    return _xor(b"\0\0" + struct.pack(">IIH", ssrc, roc, seq), ks)


def protect_packet(keys, rtp, roc):
    hdr = S.header_bytes(rtp)
    ssrc, seq = struct.unpack(">I", rtp[8:12])[0], struct.unpack(">H", rtp[2:4])[0]
    ct, tag = gcm_encrypt(keys["ke"], rtp_iv(keys["ks"], ssrc, roc, seq), rtp[:hdr], rtp[hdr:])
    return rtp[:hdr] + ct + tag


def unprotect_packet(ses, state, d):
    """one received datagram against the receiver state -> (verdict, the RTP packet or None, stream, index): srtp_model's rule, with
    T = 16 and the AEAD for a stream under a GCM rx key"""
    if len(d) < 12 + S.MIN_TAG:
        return "malformed", None, -1, -1
    by_ssrc = {c["ssrc"]: s for s, c in ses["streams"].items()}
    stream = by_ssrc.get(struct.unpack(">I", d[8:12])[0], -1)
    k = ses.get("srtp", {}).get(stream) if stream >= 0 else None
    if not (k and k.get("gcm") and _has(k, "rx")):
        return S.unprotect_packet(ses, state, d)
    body = d[:len(d) - TAG]
    hdr = S.header_bytes(body)
    if hdr is None:
        return "malformed", None, -1, -1
    keys = _keys_of(k, "rx")
    seq = struct.unpack(">H", d[2:4])[0]
    index = S.guess_index(state[stream], seq)
    pt = gcm_decrypt(keys["ke"], rtp_iv(keys["ks"], struct.unpack(">I", d[8:12])[0], index >> 16, seq), body[:hdr], body[hdr:], d[len(d) - TAG:])
    if pt is None:
        return "auth_failed", None, stream, -1
    return "ok", body[:hdr] + pt, stream, index


# ---- SRTP, the calls --------------------------------------------------------------------------------------------------------------------------------
def model_protect(ses, records, n_records, dgrams, wire, max_records=None, wire_bytes=None):
    """what solo_srtp_protect makes of pack's outputs in a session of both transforms -> dict(dgrams, wire, count)"""
    records, dgrams = np.asarray(records), np.array(dgrams, np.int32).reshape(-1, 2)
    wire = np.array(wire, np.uint8)
    wire_bytes = wire.size if wire_bytes is None else wire_bytes
    max_records = records.shape[0] if max_records is None else max_records
    count = dict.fromkeys(S.VERDICTS + ("reserved0", "reserved1"), 0)
    if n_records < 0:
        count["ok"] = -1
        return dict(dgrams=dgrams, wire=wire, count=count)
    for k in range(min(n_records, max_records)):
        off, ln = (int(v) for v in dgrams[k])
        stream, seq, desc = (int(v) for v in records[k][:3])
        if ln == 0:
            count["skipped"] += 1
            continue
        dgrams[k] = (0, 0)
        kk = ses.get("srtp", {}).get(stream)
        rtp = bytes(wire[off:off + ln]) if off >= 0 else b""
        if ln < 12 or off < 0 or off + ln > wire_bytes or stream not in range(ses["n_streams"]) or seq < 0 or desc not in (0, 1):
            count["malformed"] += 1
        elif not _has(kk, "tx"):
            count["no_key"] += 1
        elif S.header_bytes(rtp) is None or off + ln + kk["tag"] > wire_bytes:
            count["malformed"] += 1
        else:
            index = ses["streams"][stream]["seq_offset"] + 2 * seq + desc
            roc = (index >> 16) % 2 ** 32
            out = protect_packet(_keys_of(kk, "tx"), rtp, roc) if kk.get("gcm") else S.protect_packet(S.session_keys(kk["tx"]), kk["tag"], rtp, roc)
            wire[off:off + len(out)] = np.frombuffer(out, np.uint8)
            dgrams[k] = (off, len(out))
            count["ok"] += 1
    return dict(dgrams=dgrams, wire=wire, count=count)


def model_unprotect(ses, state, dgrams, wire, wire_bytes=None):
    """the BATCH receiver of the interface (srtp_model._receive with this module's packet rule)"""
    dgrams = np.asarray(dgrams, np.int32).reshape(-1, 2)
    wire = np.array(wire, np.uint8)
    wire_bytes = min(wire.size if wire_bytes is None else wire_bytes, 2 ** 31 - 1)
    out = np.zeros_like(dgrams)
    count = dict.fromkeys(S.VERDICTS + ("reserved0", "reserved1"), 0)
    verdicts, best = [], {}
    work = {s: dict(v) for s, v in state.items()}
    for i, (off, ln) in enumerate(dgrams.tolist()):
        if off < 0 or ln < 0 or off + ln > wire_bytes:
            v, rtp, stream, index = "malformed", None, -1, -1
        else:
            v, rtp, stream, index = unprotect_packet(ses, state, bytes(wire[off:off + ln]))
        verdicts.append(v)
        count[v] += 1
        if v == "ok":
            wire[off:off + len(rtp)] = np.frombuffer(rtp, np.uint8)
            out[i] = (off, len(rtp))
            best[stream] = max(best.get(stream, -1), index)
    for s, index in best.items():
        work[s]["index"] = max(work[s]["index"], index)
    return dict(dgrams=out, wire=wire, count=count, verdicts=verdicts, state=work)


# ---- SRTCP ---------------------------------------------------------------------------------------------------------------------------------------
def rtcp_iv(ks, ssrc, index):
    return _xor(b"\0\0" + struct.pack(">IHI", ssrc, 0, index), ks)


def protect_rtcp_packet(keys, rtcp, index, e=1):
    """a compound packet (at least 8 bytes) and its 31-bit index -> the datagram: [0, 8), ciphertext, tag, word; e = 0: packet, tag, word"""
    ssrc = struct.unpack(">I", rtcp[4:8])[0]
    word = struct.pack(">I", (e << 31) | index)
    iv = rtcp_iv(keys["ks"], ssrc, index)
    if e:
        ct, tag = gcm_encrypt(keys["ke"], iv, rtcp[:8] + word, rtcp[8:])
        return rtcp[:8] + ct + tag + word
    return rtcp + gcm_encrypt(keys["ke"], iv, rtcp + word, b"")[1] + word


def unprotect_rtcp_packet(keys, d):
    """a datagram of at least 8 + 20 bytes under known keys -> (authentic?, the compound packet, index)"""
    body, tag, word = d[:-RTCP_TRAILER], d[-RTCP_TRAILER:-4], d[-4:]
    w = struct.unpack(">I", word)[0]
    index = w & (C.INDEX_END - 1)
    iv = rtcp_iv(keys["ks"], struct.unpack(">I", d[4:8])[0], index)
    if w >> 31:
        pt = gcm_decrypt(keys["ke"], iv, body[:8] + word, body[8:], tag)
        return pt is not None, None if pt is None else body[:8] + pt, index
    return gcm_decrypt(keys["ke"], iv, body + word, b"", tag) is not None, body, index


def _rtcp_keys(k, d):
    return _keys_of(k, d, 3)


def model_protect_rtcp(keys, tx_state, n_streams, streams, build_refused, dgrams, wire, wire_bytes=None):
    """srtcp_model.model_protect in a session of both transforms -> dict(dgrams, wire, count, tx_state)"""
    dgrams, wire = np.array(dgrams, np.int32).reshape(-1, 2), np.array(wire, np.uint8)
    wire_bytes = min(wire.size if wire_bytes is None else wire_bytes, 2 ** 31 - 1)
    count, tx_state = dict.fromkeys(C.VERDICTS, 0), dict(tx_state)
    if build_refused:
        return dict(dgrams=dgrams, wire=wire, count=dict(count, ok=-1), tx_state=tx_state)
    for i, s in enumerate(int(v) for v in streams):
        off, ln = (int(v) for v in dgrams[i])
        if ln == 0:
            count["skipped"] += 1
            continue
        dgrams[i] = (0, 0)
        k = keys.get(s)
        gcm = bool(k and k.get("gcm") and _has(k, "tx"))
        if ln < C.HEAD or ln % 4 or off < 0 or off + ln + (RTCP_TRAILER if gcm else C.TRAILER) > wire_bytes or not 0 <= s < n_streams:
            count["malformed"] += 1
        elif not _has(k, "tx"):
            count["no_key"] += 1
        elif tx_state.get(s, 0) >= C.INDEX_END:
            count["exhausted"] += 1
        else:
            pkt = bytes(wire[off:off + ln])
            out = protect_rtcp_packet(_rtcp_keys(k, "tx"), pkt, tx_state.get(s, 0)) if gcm else C.protect_packet(C.session_keys(k["tx"]), pkt, tx_state.get(s, 0))
            wire[off:off + len(out)] = np.frombuffer(out, np.uint8)
            dgrams[i] = (off, len(out))
            tx_state[s] = tx_state.get(s, 0) + 1
            count["ok"] += 1
    return dict(dgrams=dgrams, wire=wire, count=count, tx_state=tx_state)


def model_unprotect_rtcp(session, keys, rx_state, dgrams, wire, wire_bytes=None):
    """the BATCH receiver: srtcp_model's rules; a datagram of a GCM-keyed stream below 8 + 20 bytes is malformed once its key is known"""
    dgrams, wire = np.asarray(dgrams, np.int32).reshape(-1, 2), np.array(wire, np.uint8)
    wire_bytes = min(wire.size if wire_bytes is None else wire_bytes, 2 ** 31 - 1)
    out, count, verdicts = np.zeros_like(dgrams), dict.fromkeys(C.VERDICTS, 0), []
    work, best = dict(rx_state), {}
    for i, (off, ln) in enumerate(dgrams.tolist()):
        d = bytes(wire[off:off + ln]) if off >= 0 and ln >= 0 and off + ln <= wire_bytes else None
        stream = session.find(struct.unpack(">I", d[4:8])[0]) if d is not None and len(d) >= C.HEAD + C.TRAILER else -1
        k = keys.get(stream)
        if d is None or len(d) < C.HEAD + C.TRAILER:
            v = "malformed"
        elif stream < 0:
            v = "unknown_ssrc"
        elif not _has(k, "rx"):
            v = "no_key"
        elif k.get("gcm") and len(d) < C.HEAD + RTCP_TRAILER:
            v = "malformed"
        else:
            good, plain, index = unprotect_rtcp_packet(_rtcp_keys(k, "rx"), d) if k.get("gcm") else C.unprotect_packet(C.session_keys(k["rx"]), d)
            if index <= rx_state.get(stream, -1):
                v = "replayed"
            elif not good:
                v = "auth_failed"
            else:
                v = "ok"
                wire[off:off + len(plain)] = np.frombuffer(plain, np.uint8)
                out[i] = (off, len(plain))
                best[stream] = max(best.get(stream, -1), index)
        verdicts.append(v)
        count[v] += 1
    for s, index in best.items():
        work[s] = max(work.get(s, -1), index)
    return dict(dgrams=out, wire=wire, count=count, verdicts=verdicts, rx_state=work)


# ---- inputs both test files share ----------------------------------------------------------------------------------------------------------------
LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 300]      # plaintext lengths: the block edges, a row's second keystream block, > 16 GHASH blocks


def random_master(rng):
    return rng.integers(0, 256, MASTER, dtype=np.uint8).tobytes()


def gcm_entry(rng, tx=True, rx=True):
    return dict(tx=random_master(rng) if tx else None, rx=random_master(rng) if rx else None, tag=TAG, gcm=True)


def loop_session(ses):
    """the receiving end of ses: the same bindings, every stream's rx key = the sender's tx key, whichever transform"""
    return dict(ses, srtp={s: dict(k, tx=None, rx=k["tx"]) for s, k in ses["srtp"].items()})


def hostile_set(ses, state, stream, rng, rtp_model):
    """GCM datagrams of `stream` (bound, GCM rx key) -> [(name, bytes, verdict)]: valid ones with sequence numbers near the state's, each
    once, and what must be rejected"""
    c, k = ses["streams"][stream], ses["srtp"][stream]
    keys = _keys_of(k, "rx")
    st = state[stream]
    base = st["index"] if st["index"] >= 0 else (st["roc0"] << 16) | 1000
    seqs = iter(range(1, 60))

    def rtp(n=None, **kw):
        index = base + next(seqs)
        pl = rng.integers(0, 256, int(rng.integers(1, 80)) if n is None else n, dtype=np.uint8).tobytes()
        return rtp_model.build(c["ssrc"], c["pt"][0], index & 0xFFFF, int(rng.integers(0, 2 ** 32)), pl, **kw), index >> 16

    def good(n=None, **kw):
        p, roc = rtp(n, **kw)
        return protect_packet(keys, p, roc)

    def flip(d, at, bit=0x10):
        return d[:at] + bytes([d[at] ^ bit]) + d[at + 1:]

    out = [("plain", good(), "ok"), ("one_byte", good(1), "ok"), ("csrc", good(csrc=[7, 8, 9]), "ok"),
           ("level", good(ext=rtp_model.level_ext(ses["level_id"] or 1, 0x55)), "ok"), ("long", good(300), "ok"), ("empty_payload", good(0), "ok")]
    d = good(40)
    out += [("flip_header", flip(d, 1, 0x80), "auth_failed"), ("flip_seq", flip(d, 3, 0x01), "auth_failed"), ("flip_payload", flip(d, 30), "auth_failed"),
            ("flip_tag", flip(d, len(d) - 1), "auth_failed"), ("flip_tag_first", flip(d, len(d) - TAG), "auth_failed"),
            ("one_byte_cut", d[:-1], "auth_failed"), ("extended", d + b"\x00", "auth_failed")]
    p, roc = rtp(33)
    out.append(("wrong_roc", protect_packet(keys, p, (roc + 1) % 2 ** 32), "auth_failed"))
    out.append(("wrong_key", protect_packet(session_keys(bytes(MASTER)), rtp(20)[0], roc), "auth_failed"))
    out.append(("other_transform", S.protect_packet(S.session_keys(bytes(30)), 10, rtp(20)[0], roc), "auth_failed"))
    p, roc = rtp(2)
    d = protect_packet(keys, p, roc)
    out.append(("cc_into_tag", bytes([d[0] | 1]) + d[1:], "malformed"))                                       # 12 + 4 > 14
    d = good(1)
    out += [("len_27", d[:12 + TAG - 1], "malformed"), ("len_16", d[:12 + S.MIN_TAG], "malformed"), ("len_15", d[:15], "malformed")]
    return out

"""An independent model of the SRTP stage (solo_srtp_protect / solo_srtp_unprotect, include/solo_mi355x.h), written from RFC 3711 -- not from
the HIP source.  AES-128 is FIPS-197 written out plainly: the S-box from the field inverse and the affine map, SubBytes / ShiftRows /
MixColumns on a 16-byte state, no T-tables.  HMAC-SHA1 is hashlib / hmac.  Key derivation (section 4.3, rate 0), the AES-CM keystream
(4.1.1), protect, the SEQUENTIAL receiver of section 3.3 / appendix A (one datagram after another, the state moving with each), and as a
second function the BATCH receiver of the interface (every datagram of a call judged against the state the call began with).

A session is rtp_model's dict plus ses["srtp"] = {stream: dict(tx=master30 or None, rx=master30 or None, tag=10 or 4)}; a receiver state
is {stream: dict(index=-1 or the highest authenticated index, roc0=the initial rollover counter)}."""
import functools
import hashlib
import hmac
import struct

import numpy as np

VERDICTS = ("ok", "skipped", "malformed", "unknown_ssrc", "no_key", "auth_failed")
MIN_TAG = 4            # the tag the `malformed` rule assumes where the stream, or its rx key, is not known


# ---- AES-128 (FIPS-197) -------------------------------------------------------------------------------------------------------------------
def _xtime(a):
    a <<= 1
    return (a ^ 0x11B) & 0xFF if a & 0x100 else a


def _gmul(a, b):
    r = 0
    while b:
        if b & 1:
            r ^= a
        a, b = _xtime(a), b >> 1
    return r


def _make_sbox():
    inv = [0] * 256
    for a in range(1, 256):
        inv[a] = next(b for b in range(1, 256) if _gmul(a, b) == 1)
    box = []
    for a in range(256):
        x, y = inv[a], inv[a]
        for _ in range(4):
            y = ((y << 1) | (y >> 7)) & 0xFF
            x ^= y
        box.append(x ^ 0x63)
    return box


SBOX = _make_sbox()


@functools.lru_cache(maxsize=256)
def aes_expand(key):
    w = [list(key[4 * i:4 * i + 4]) for i in range(4)]
    rcon = 1
    for i in range(4, 44):
        t = list(w[i - 1])
        if i % 4 == 0:
            t = [SBOX[b] for b in t[1:] + t[:1]]
            t[0] ^= rcon
            rcon = _xtime(rcon)
        w.append([a ^ b for a, b in zip(w[i - 4], t)])
    return [sum(w[4 * r:4 * r + 4], []) for r in range(11)]


def aes_encrypt(key, block):
    rk = aes_expand(bytes(key))
    s = [a ^ b for a, b in zip(block, rk[0])]
    for r in range(1, 11):
        s = [SBOX[b] for b in s]
        s = [s[(4 * c + row + 4 * row) % 16] for c in range(4) for row in range(4)]            # ShiftRows: row `row` moves left by `row` columns
        if r < 10:
            m = []
            for c in range(4):
                a = s[4 * c:4 * c + 4]
                m += [_gmul(a[0], 2) ^ _gmul(a[1], 3) ^ a[2] ^ a[3], a[0] ^ _gmul(a[1], 2) ^ _gmul(a[2], 3) ^ a[3],
                      a[0] ^ a[1] ^ _gmul(a[2], 2) ^ _gmul(a[3], 3), _gmul(a[0], 3) ^ a[1] ^ a[2] ^ _gmul(a[3], 2)]
            s = m
        s = [a ^ b for a, b in zip(s, rk[r])]
    return bytes(s)


def aes_cm(key, iv, n, first_block=0):
    """n bytes of keystream: AES(key, (IV + j) mod 2^128) for j = first_block, ..."""
    out, j = b"", first_block
    while len(out) < n:
        out += aes_encrypt(key, ((iv + j) % 2 ** 128).to_bytes(16, "big"))
        j += 1
    return out[:n]


# ---- key derivation (RFC 3711 section 4.3, key derivation rate 0) ----------------------------------------------------------------------------
def derive(master_key, master_salt, label, n):
    x = int.from_bytes(master_salt, "big") ^ (label << 48)        # key_id = label || r, r = index DIV rate = 0
    return aes_cm(master_key, x << 16, n)


@functools.lru_cache(maxsize=256)
def session_keys(master30):
    mk, ms = bytes(master30[:16]), bytes(master30[16:30])
    return dict(ke=derive(mk, ms, 0, 16), ka=derive(mk, ms, 1, 20), ks=derive(mk, ms, 2, 14))


# ---- the RTP header ---------------------------------------------------------------------------------------------------------------------------
def header_bytes(d):
    """bytes in front of the payload of the RTP packet d: 12 + 4 CC and the extension block; None where that reaches past the end"""
    if len(d) < 12:
        return None
    hdr = 12 + 4 * (d[0] & 15)
    if hdr > len(d):
        return None
    if d[0] & 0x10:
        if hdr + 4 > len(d):
            return None
        hdr += 4 + 4 * struct.unpack(">H", d[hdr + 2:hdr + 4])[0]
        if hdr > len(d):
            return None
    return hdr


# ---- one packet ---------------------------------------------------------------------------------------------------------------------------------
def protect_packet(keys, tag_bytes, rtp, roc):
    """an RTP packet (bytes, a well-formed header) and the sender's rollover counter -> the SRTP packet"""
    hdr = header_bytes(rtp)
    ssrc, seq = struct.unpack(">I", rtp[8:12])[0], struct.unpack(">H", rtp[2:4])[0]
    index = (roc << 16) | seq
    iv = (int.from_bytes(keys["ks"], "big") << 16) ^ (ssrc << 64) ^ (index << 16)
    body = rtp[:hdr] + bytes(a ^ b for a, b in zip(rtp[hdr:], aes_cm(keys["ke"], iv, len(rtp) - hdr)))
    return body + hmac.new(keys["ka"], body + struct.pack(">I", roc), hashlib.sha1).digest()[:tag_bytes]


def guess_index(state, seq):
    """RFC 3711 section 3.3.1 / appendix A against state = dict(index, roc0)"""
    if state["index"] < 0:
        v = state["roc0"]
    else:
        roc, s_l = state["index"] >> 16, state["index"] & 0xFFFF
        if s_l < 32768:
            v = (roc - 1) % 2 ** 32 if seq - s_l > 32768 else roc
        else:
            v = (roc + 1) % 2 ** 32 if s_l - 32768 > seq else roc
    return (v << 16) | seq


def unprotect_packet(ses, state, d):
    """one received datagram against the receiver state -> (verdict, the RTP packet or None, stream, index)"""
    by_ssrc = {c["ssrc"]: s for s, c in ses["streams"].items()}
    if len(d) < 12 + MIN_TAG:
        return "malformed", None, -1, -1
    stream = by_ssrc.get(struct.unpack(">I", d[8:12])[0], -1)
    k = ses["srtp"].get(stream) if stream >= 0 else None
    key = k["rx"] if k and k.get("rx") is not None else None
    tag = k["tag"] if key is not None else MIN_TAG
    body = d[:len(d) - tag]
    hdr = header_bytes(body)
    if hdr is None:
        return "malformed", None, -1, -1
    if stream < 0:
        return "unknown_ssrc", None, -1, -1
    if key is None:
        return "no_key", None, stream, -1
    keys = session_keys(key)
    seq = struct.unpack(">H", d[2:4])[0]
    index = guess_index(state[stream], seq)
    roc = index >> 16
    if not hmac.compare_digest(hmac.new(keys["ka"], body + struct.pack(">I", roc), hashlib.sha1).digest()[:tag], d[len(d) - tag:]):
        return "auth_failed", None, stream, -1
    iv = (int.from_bytes(keys["ks"], "big") << 16) ^ (struct.unpack(">I", d[8:12])[0] << 64) ^ (index << 16)
    return "ok", body[:hdr] + bytes(a ^ b for a, b in zip(body[hdr:], aes_cm(keys["ke"], iv, len(body) - hdr))), stream, index


def new_state(ses, roc0=None):
    return {s: dict(index=-1, roc0=(roc0 or {}).get(s, 0)) for s in range(ses["n_streams"])}


# ---- the calls ------------------------------------------------------------------------------------------------------------------------------------
def model_protect(ses, records, n_records, dgrams, wire, max_records=None, wire_bytes=None):
    """what solo_srtp_protect makes of pack's outputs: -> dict(dgrams, wire, count)"""
    records, dgrams = np.asarray(records), np.array(dgrams, np.int32).reshape(-1, 2)
    wire = np.array(wire, np.uint8)
    wire_bytes = wire.size if wire_bytes is None else wire_bytes
    max_records = records.shape[0] if max_records is None else max_records
    count = dict.fromkeys(VERDICTS + ("reserved0", "reserved1"), 0)
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
        elif not kk or kk.get("tx") is None:
            count["no_key"] += 1
        elif header_bytes(rtp) is None or off + ln + kk["tag"] > wire_bytes:
            count["malformed"] += 1
        else:
            index = ses["streams"][stream]["seq_offset"] + 2 * seq + desc          # the unreduced integer behind pack's sequence number
            assert index % 65536 == struct.unpack(">H", rtp[2:4])[0]
            out = protect_packet(session_keys(kk["tx"]), kk["tag"], rtp, (index >> 16) % 2 ** 32)
            wire[off:off + len(out)] = np.frombuffer(out, np.uint8)
            dgrams[k] = (off, len(out))
            count["ok"] += 1
    return dict(dgrams=dgrams, wire=wire, count=count)


def _receive(ses, state, dgrams, wire, wire_bytes, sequential):
    dgrams = np.asarray(dgrams, np.int32).reshape(-1, 2)
    wire = np.array(wire, np.uint8)
    wire_bytes = min(wire.size if wire_bytes is None else wire_bytes, 2 ** 31 - 1)
    out = np.zeros_like(dgrams)
    count = dict.fromkeys(VERDICTS + ("reserved0", "reserved1"), 0)
    verdicts, best = [], {}
    work = {s: dict(v) for s, v in state.items()}
    for i, (off, ln) in enumerate(dgrams.tolist()):
        if off < 0 or ln < 0 or off + ln > wire_bytes:
            v, rtp, stream, index = "malformed", None, -1, -1
        else:
            v, rtp, stream, index = unprotect_packet(ses, work if sequential else state, bytes(wire[off:off + ln]))
        verdicts.append(v)
        count[v] += 1
        if v == "ok":
            wire[off:off + len(rtp)] = np.frombuffer(rtp, np.uint8)
            out[i] = (off, len(rtp))
            if sequential:
                work[stream]["index"] = max(work[stream]["index"], index)      # appendix A: s_l and ROC move only forward
            else:
                best[stream] = max(best.get(stream, -1), index)
    if not sequential:
        for s, index in best.items():
            work[s]["index"] = max(work[s]["index"], index)
    return dict(dgrams=out, wire=wire, count=count, verdicts=verdicts, state=work)


def model_unprotect(ses, state, dgrams, wire, wire_bytes=None):
    """the BATCH receiver of the interface -> dict(dgrams (out), wire, count, verdicts, state (after the call))"""
    return _receive(ses, state, dgrams, wire, wire_bytes, False)


def sequential_unprotect(ses, state, dgrams, wire, wire_bytes=None):
    """the receiver of the RFC, datagram after datagram"""
    return _receive(ses, state, dgrams, wire, wire_bytes, True)


def model_pack_trailer(rtp_model, ses, records, n_records, payload, level, trailer, max_records=None, cap=None):
    """solo_rtp_pack with a trailer of T bytes, out of rtp_model.model_pack (which knows none): the same datagrams, each followed by T
    zero bytes and then the pad bytes up to a multiple of 4; dgrams[k].len stays the RTP packet's -> dict(dgrams, wire, count)"""
    full = rtp_model.model_pack(ses, records, n_records, payload, level, max_records, None)
    cap = 2 ** 31 - 1 if cap is None else min(cap, 2 ** 31 - 1)
    src, wire, dg = full["all_wire"], bytearray(), np.zeros_like(full["all_dgrams"])
    need, written, nbytes = 0, 0, 0
    for k, (off, ln) in enumerate(full["all_dgrams"].tolist()):
        if ln == 0:
            continue
        padded = (ln + trailer + 3) & ~3
        if need + padded <= cap:
            dg[k] = (need, ln)
            wire += bytes(src[off:off + ln]) + b"\x00" * (padded - ln)
            written, nbytes = written + 1, need + padded
        need += padded
    count = dict(full["count"], dgrams=written, bytes=nbytes, bytes_needed=need)
    return dict(dgrams=dg, wire=np.frombuffer(bytes(wire), np.uint8), count=count)


# ---- inputs both test files share ----------------------------------------------------------------------------------------------------------------
def random_keys(rng, ses, tag=10, no_tx=(), no_rx=()):
    """ses["srtp"]: every bound stream gets two random masters (but `no_tx` / `no_rx`)"""
    ses["srtp"] = {s: dict(tx=None if s in no_tx else rng.integers(0, 256, 30, dtype=np.uint8).tobytes(),
                           rx=None if s in no_rx else rng.integers(0, 256, 30, dtype=np.uint8).tobytes(), tag=tag) for s in ses["streams"]}
    return ses


def loop_session(ses):
    """the receiving end of ses: the same bindings, every stream's rx key = the sender's tx key"""
    return dict(ses, srtp={s: dict(tx=None, rx=k["tx"], tag=k["tag"]) for s, k in ses["srtp"].items()})


# payload lengths: the cipher's block edges, then those that put the authenticated length M = H + len + 4 on the SHA-1 padding edges
# (M mod 64 in {54, 55, 56, 63, 0, 1}), for H = 12 and H = 20
def edge_lengths(H):
    return [1, 15, 16, 17, 33, 252] + [M - H - 4 for M in (118, 119, 120, 127, 128, 129)]


def hostile_set(ses, state, stream, rng, rtp_model):
    """SRTP datagrams of `stream` (bound, rx key set, distinct payload types) that must be rejected, and valid ones beside them ->
    [(name, bytes, verdict)].  The valid ones use sequence numbers near the state's, each once."""
    c, k = ses["streams"][stream], ses["srtp"][stream]
    keys, tag = session_keys(k["rx"]), k["tag"]
    st = state[stream]
    base = st["index"] if st["index"] >= 0 else (st["roc0"] << 16) | 1000
    seqs = iter(range(1, 60))

    def rtp(n=None, **kw):
        index = base + next(seqs)
        pl = rng.integers(0, 256, int(rng.integers(1, 80)) if n is None else n, dtype=np.uint8).tobytes()
        return rtp_model.build(c["ssrc"], c["pt"][0], index & 0xFFFF, int(rng.integers(0, 2 ** 32)), pl, **kw), index >> 16

    def good(n=None, **kw):
        p, roc = rtp(n, **kw)
        return protect_packet(keys, tag, p, roc)

    def flip(d, at, bit=0x10):
        return d[:at] + bytes([d[at] ^ bit]) + d[at + 1:]

    other = dict(c, ssrc=c["ssrc"] ^ 0x5A5A5A5A)
    out = [("plain", good(), "ok"), ("one_byte", good(1), "ok"), ("csrc", good(csrc=[7, 8, 9]), "ok"),
           ("level", good(ext=rtp_model.level_ext(ses["level_id"] or 1, 0x55)), "ok"), ("long", good(252), "ok")]
    d = good(40)
    out += [("flip_header", flip(d, 1, 0x80), "auth_failed"), ("flip_seq", flip(d, 3, 0x01), "auth_failed"), ("flip_payload", flip(d, 30), "auth_failed"),
            ("flip_tag", flip(d, len(d) - 1), "auth_failed"), ("flip_tag_first", flip(d, len(d) - tag), "auth_failed"),
            ("truncated_tag", d[:-1], "auth_failed"), ("extended", d + b"\x00", "auth_failed")]
    p, roc = rtp(33)
    out.append(("wrong_roc", protect_packet(keys, tag, p, (roc + 1) % 2 ** 32), "auth_failed"))
    out.append(("other_key", protect_packet(session_keys(bytes(30)), tag, rtp(20)[0], roc), "auth_failed"))
    # CC or the extension length reaching into the tag: the header walk runs over len - tag bytes
    p, roc = rtp(2)
    d = protect_packet(keys, tag, p, roc)
    out.append(("cc_into_tag", bytes([d[0] | 1]) + d[1:], "malformed"))                                     # 12 + 4 > 14
    p, roc = rtp(1, ext=rtp_model.extension_block(0xBEDE, b"", length_words=0))
    d = protect_packet(keys, tag, p, roc)
    out.append(("ext_into_tag", d[:14] + b"\x00\x01" + d[16:], "malformed"))                                  # the block now claims 4 more bytes than len - tag has
    d = good(3)
    out.append(("x_no_room", bytes([d[0] | 0x10]) + d[1:], "malformed"))                                      # 12 + 4 > 15: no room for the block's first word
    out += [("short", good(1)[:12 + tag - 1], "malformed"), ("eleven", good(1)[:11], "malformed"), ("empty_payload", good(1)[:12] + good(1)[-tag:], "auth_failed")]
    unknown = rtp_model.build(other["ssrc"], c["pt"][0], 5, 0, b"abcdefgh" * 3)
    out += [("unknown_ssrc", unknown, "unknown_ssrc"), ("unknown_ssrc_short", unknown[:12 + MIN_TAG], "unknown_ssrc"),
            ("unknown_ssrc_too_short", unknown[:12 + MIN_TAG - 1], "malformed")]
    return out

"""An independent model of the SRTCP stage (solo_srtcp_protect / solo_srtcp_unprotect, solo_rtcp_set_trailer; include/solo_mi355x.h),
written from RFC 3711 section 3.4 -- not from the HIP source.  It stands on the pieces of tests/srtp_model.py, which published answers
pin (the plain FIPS-197 AES, the AES-CM keystream, the PRF of section 4.3; HMAC-SHA1 is hashlib / hmac): key derivation with labels
3 / 4 / 5, one packet out and in, protect with its per-stream send index, a SEQUENTIAL receiver (one datagram after another under the
strictly-newer rule) and the BATCH receiver of the interface (every datagram of a call judged against the records the call began with).

keys = {stream: dict(tx=master30 or None, rx=master30 or None)}; tx_state = {stream: the index the next protected packet gets};
rx_state = {stream: the highest authenticated index, -1 = none yet}; a session is an rtcp_model.Session (its find() is the SSRC table)."""
import functools
import hashlib
import hmac
import struct

import numpy as np

import srtp_model as S

VERDICTS = ("ok", "skipped", "malformed", "unknown_ssrc", "no_key", "auth_failed", "replayed", "exhausted")
TAG = 10                # HMAC_SHA1_80, in every suite (RFC 3711 section 5.2, RFC 4568)
TRAILER = 4 + TAG       # E || index, then the tag; no MKI
HEAD = 8                # the first header and the sender SSRC stay in the clear
INDEX_END = 2 ** 31


@functools.lru_cache(maxsize=512)
def session_keys(master30):
    mk, ms = bytes(master30[:16]), bytes(master30[16:30])
    return dict(ke=S.derive(mk, ms, 3, 16), ka=S.derive(mk, ms, 4, 20), ks=S.derive(mk, ms, 5, 14))


def _iv(keys, ssrc, index):
    return (int.from_bytes(keys["ks"], "big") << 16) ^ (ssrc << 64) ^ (index << 16)


def protect_packet(keys, rtcp, index, e=1):
    """a compound packet (bytes, at least 8) and its 31-bit index -> the SRTCP datagram; e = 0: authenticated only"""
    ssrc = struct.unpack(">I", rtcp[4:8])[0]
    body = rtcp
    if e:
        body = rtcp[:HEAD] + bytes(a ^ b for a, b in zip(rtcp[HEAD:], S.aes_cm(keys["ke"], _iv(keys, ssrc, index), len(rtcp) - HEAD)))
    word = struct.pack(">I", (e << 31) | index)
    return body + word + hmac.new(keys["ka"], body + word, hashlib.sha1).digest()[:TAG]


def unprotect_packet(keys, d):
    """an SRTCP datagram of at least 8 + 14 bytes under known keys -> (authentic?, the compound packet, index)"""
    body, word, tag = d[:-TRAILER], d[-TRAILER:-TAG], d[-TAG:]
    w = struct.unpack(">I", word)[0]
    index = w & (INDEX_END - 1)
    if not hmac.compare_digest(hmac.new(keys["ka"], body + word, hashlib.sha1).digest()[:TAG], tag):
        return False, None, index
    if w >> 31:
        ssrc = struct.unpack(">I", d[4:8])[0]
        body = body[:HEAD] + bytes(a ^ b for a, b in zip(body[HEAD:], S.aes_cm(keys["ke"], _iv(keys, ssrc, index), len(body) - HEAD)))
    return True, body, index


# ---- build with a trailer ---------------------------------------------------------------------------------------------------------------------
def model_build_trailer(model, tx, rx, streams, now, cap, trailer):
    """solo_rtcp_build with a trailer of T bytes, out of rtcp_model.Model.build (which knows none): the same packets, each followed by T
    zero bytes and the pad up to a multiple of 4; dgrams[i].len stays the packet's; a packet is written iff it ends, trailer included,
    inside cap, and only a written packet moves the state -> (refused call?, dgrams, wire bytes, count)"""
    import copy
    refused, dg, wire, c = copy.deepcopy(model).build(tx, rx, streams, now, 2 ** 31 - 1)
    if refused:
        return model.build(tx, rx, streams, now, cap)
    cap = min(cap, 2 ** 31 - 1)
    out, w, need, fit = [], bytearray(), 0, 0
    for off, ln in dg:
        padded = (ln + trailer + 3) & ~3 if ln else 0
        if ln and need + padded <= cap:
            out.append((need, ln))
            w += wire[off:off + ln] + b"\0" * (padded - ln)
            fit += ln
        else:
            out.append((0, 0))
        need += padded
    _, _, _, c2 = model.build(tx, rx, streams, now, fit)       # (the written packets are a prefix: a cap of their own bytes writes exactly them)
    assert c2["bytes"] == fit
    return False, out, bytes(w), dict(c2, bytes=len(w), bytes_needed=need)


# ---- the calls ------------------------------------------------------------------------------------------------------------------------------------
def model_protect(keys, tx_state, n_streams, streams, build_refused, dgrams, wire, wire_bytes=None):
    """-> dict(dgrams, wire, count, tx_state (after the call))"""
    dgrams, wire = np.array(dgrams, np.int32).reshape(-1, 2), np.array(wire, np.uint8)
    wire_bytes = min(wire.size if wire_bytes is None else wire_bytes, 2 ** 31 - 1)
    count, tx_state = dict.fromkeys(VERDICTS, 0), dict(tx_state)
    if build_refused:
        return dict(dgrams=dgrams, wire=wire, count=dict(count, ok=-1), tx_state=tx_state)
    for i, s in enumerate(int(v) for v in streams):
        off, ln = (int(v) for v in dgrams[i])
        if ln == 0:
            count["skipped"] += 1
            continue
        dgrams[i] = (0, 0)
        k = keys.get(s)
        if ln < HEAD or ln % 4 or off < 0 or off + ln + TRAILER > wire_bytes or not 0 <= s < n_streams:
            count["malformed"] += 1
        elif not k or k.get("tx") is None:
            count["no_key"] += 1
        elif tx_state.get(s, 0) >= INDEX_END:
            count["exhausted"] += 1
        else:
            out = protect_packet(session_keys(k["tx"]), bytes(wire[off:off + ln]), tx_state.get(s, 0))
            wire[off:off + len(out)] = np.frombuffer(out, np.uint8)
            dgrams[i] = (off, len(out))
            tx_state[s] = tx_state.get(s, 0) + 1
            count["ok"] += 1
    return dict(dgrams=dgrams, wire=wire, count=count, tx_state=tx_state)


def _receive(session, keys, rx_state, dgrams, wire, wire_bytes, sequential):
    dgrams, wire = np.asarray(dgrams, np.int32).reshape(-1, 2), np.array(wire, np.uint8)
    wire_bytes = min(wire.size if wire_bytes is None else wire_bytes, 2 ** 31 - 1)
    out, count, verdicts = np.zeros_like(dgrams), dict.fromkeys(VERDICTS, 0), []
    work, best = dict(rx_state), {}
    for i, (off, ln) in enumerate(dgrams.tolist()):
        d = bytes(wire[off:off + ln]) if off >= 0 and ln >= 0 and off + ln <= wire_bytes else None
        stream = session.find(struct.unpack(">I", d[4:8])[0]) if d is not None and len(d) >= HEAD + TRAILER else -1
        k = keys.get(stream)
        if d is None or len(d) < HEAD + TRAILER:
            v = "malformed"
        elif stream < 0:
            v = "unknown_ssrc"
        elif not k or k.get("rx") is None:
            v = "no_key"
        else:
            good, plain, index = unprotect_packet(session_keys(k["rx"]), d)
            if index <= (work if sequential else rx_state).get(stream, -1):
                v = "replayed"
            elif not good:
                v = "auth_failed"
            else:
                v = "ok"
                wire[off:off + len(plain)] = np.frombuffer(plain, np.uint8)
                out[i] = (off, len(plain))
                if sequential:
                    work[stream] = index
                else:
                    best[stream] = max(best.get(stream, -1), index)
        verdicts.append(v)
        count[v] += 1
    for s, index in best.items():
        work[s] = max(work.get(s, -1), index)
    return dict(dgrams=out, wire=wire, count=count, verdicts=verdicts, rx_state=work)


def model_unprotect(session, keys, rx_state, dgrams, wire, wire_bytes=None):
    """the BATCH receiver of the interface: "strictly newer than everything authenticated before this call" """
    return _receive(session, keys, rx_state, dgrams, wire, wire_bytes, False)


def sequential_unprotect(session, keys, rx_state, dgrams, wire, wire_bytes=None):
    """a packet-by-packet receiver under the same rule: strictly newer than everything authenticated so far"""
    return _receive(session, keys, rx_state, dgrams, wire, wire_bytes, True)


# ---- inputs both test files share ----------------------------------------------------------------------------------------------------------------
def random_keys(rng, streams, no_tx=(), no_rx=()):
    return {s: dict(tx=None if s in no_tx else rng.integers(0, 256, 30, dtype=np.uint8).tobytes(),
                    rx=None if s in no_rx else rng.integers(0, 256, 30, dtype=np.uint8).tobytes()) for s in streams}


def loop_keys(keys):
    """the receiving end: every stream's rx key = the sender's tx key"""
    return {s: dict(tx=None, rx=k["tx"]) for s, k in keys.items()}


def lay_out(rng, packets, front=None, gap=None, align=None):
    """datagrams at chosen byte alignments inside one wire buffer of random filler -> (dgrams int32 [n,2], wire uint8)"""
    wire, dg = bytearray(rng.integers(0, 256, 5 if front is None else front, dtype=np.uint8).tobytes()), []
    for i, d in enumerate(packets):
        if align is not None:
            wire += rng.integers(0, 256, (align[i % len(align)] - len(wire)) % 4, dtype=np.uint8).tobytes()
        dg.append((len(wire), len(d)))
        wire += d + rng.integers(0, 256, int(rng.integers(0, 7)) if gap is None else gap, dtype=np.uint8).tobytes()
    return np.array(dg, np.int32).reshape(-1, 2), np.frombuffer(bytes(wire), np.uint8).copy()


def foreign_shapes(R, rng, ssrc, other_ssrc):
    """valid compound packets the builder never writes -> [(name, bytes)]"""
    def blocks(n):
        return [R.write_block(other_ssrc + k, k, 3 * k, 70000 + k, 5 + k, 0x12340000, 77) for k in range(n)]
    app = struct.pack(">BBH", 0x80, 204, 2 + 5) + struct.pack(">I", ssrc) + b"solo" + rng.integers(0, 256, 20, dtype=np.uint8).tobytes()
    big = struct.pack(">BBH", 0x80, 204, 2 + 190) + struct.pack(">I", ssrc) + b"bulk" + rng.integers(0, 256, 760, dtype=np.uint8).tobytes()
    sdes = R.write_sdes(ssrc, b"someone@example.org")
    return [("rr_three_blocks", R.write_rr(ssrc, blocks(3)) + sdes), ("sr_two_blocks", R.write_sr(ssrc, 0x83AA7E8012345678, 99, 5, 600, blocks(2)) + sdes),
            ("bye", R.write_rr(ssrc) + sdes + R.write_bye([ssrc])), ("app", R.write_rr(ssrc) + sdes + app), ("large", R.write_rr(ssrc) + big),
            ("bare_rr", R.write_rr(ssrc)),                                            # 8 bytes: nothing to encrypt
            ("odd_9", R.write_rr(ssrc) + b"\x01"), ("odd_27", R.write_rr(ssrc) + sdes[:19]), ("odd_150", R.write_rr(ssrc) + big[:142])]


def hostile_set(R, rng, session, keys, rx_state, stream, first_index):
    """SRTCP datagrams for `stream` (bound in session, rx key set) -> [(name, bytes, verdict)]: the foreign shapes with rising indices from
    first_index (> the stream's record), then what must be rejected.  No index of an accepted datagram occurs twice but in "copy"."""
    k, ssrc = session_keys(keys[stream]["rx"]), session.ssrc[stream]
    assert first_index > rx_state.get(stream, -1)
    idx = iter(range(first_index, first_index + 100))
    out = [(name, protect_packet(k, pkt, next(idx), e=0 if name == "odd_27" else 1), "ok") for name, pkt in foreign_shapes(R, rng, ssrc, 0x77000000)]
    out.append(("e0", protect_packet(k, R.write_rr(ssrc) + R.write_sdes(ssrc, b"clear"), next(idx), e=0), "ok"))
    i = next(idx)
    d = protect_packet(k, R.write_rr(ssrc) + R.write_sdes(ssrc, b"twice"), i)
    out += [("copy_a", d, "ok"), ("copy_b", d, "ok")]

    def flip(d, at, bit=0x10):
        return d[:at] + bytes([d[at] ^ bit]) + d[at + 1:]
    d = protect_packet(k, R.write_sr(ssrc, 1 << 40, 7, 8, 9) + R.write_sdes(ssrc, b"victim"), next(idx))
    out += [("flip_tag", flip(d, len(d) - 1), "auth_failed"), ("flip_tag_first", flip(d, len(d) - TAG), "auth_failed"),
            ("flip_index", flip(d, len(d) - TRAILER + 1, 0x01), "auth_failed"), ("flip_e", flip(d, len(d) - TRAILER, 0x80), "auth_failed"),
            ("flip_body", flip(d, 20), "auth_failed"), ("other_key", protect_packet(session_keys(bytes(30)), d[:40], next(idx)), "auth_failed")]
    out += [("flip_byte_%d" % b, flip(d, b, 0x01 if b != 7 else 0x80), "auth_failed") for b in (0, 1, 2, 3)]
    # bytes 4 .. 7 are the SSRC: flipped, the datagram is nobody's -- or another stream's, whose key then fails it (twin_session below
    # binds such streams)
    for b in (4, 5, 6, 7):
        s2 = session.find(ssrc ^ (2 << (8 * (7 - b))))
        v = "unknown_ssrc" if s2 < 0 else "no_key" if keys.get(s2, {}).get("rx") is None else "replayed" if (len(d) and unprotect_packet(k, d)[2] <= rx_state.get(s2, -1)) \
            else "auth_failed"
        out.append(("flip_byte_%d" % b, flip(d, b, 0x02), v))
    rec = rx_state.get(stream, -1)
    if rec >= 0:
        out += [("equal_to_record", protect_packet(k, R.write_rr(ssrc), rec), "replayed"), ("below_record", protect_packet(k, R.write_rr(ssrc), max(rec - 3, 0)), "replayed"),
                ("replayed_and_forged", flip(protect_packet(k, R.write_rr(ssrc) + R.write_sdes(ssrc, b"old"), rec), 9), "replayed")]
    out += [("len_21", d[:21], "malformed"), ("len_22", d[:8] + d[-TRAILER:], "auth_failed"), ("len_7", d[:7], "malformed")]
    unknown = protect_packet(k, R.write_rr(ssrc ^ 0x5A5A5A5A), next(idx))
    out += [("unknown_ssrc", unknown, "unknown_ssrc"), ("unknown_ssrc_short", unknown[:21], "malformed")]
    return out


def twin_ssrcs(ssrc):
    """the four SSRCs one flipped bit (bit 1 of each byte) away from ssrc: bound to other keyed streams, a flipped SSRC byte fails the tag"""
    return [ssrc ^ (2 << (8 * k)) for k in range(4)]

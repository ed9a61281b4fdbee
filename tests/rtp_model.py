"""An independent model of solo_rtp_pack / solo_rtp_parse (include/solo_mi355x.h), written from RFC 3550 section 5.1 (the fixed header),
RFC 8285 section 4.2 (one-byte header extensions) and RFC 6464 (the audio level element) with struct and plain Python -- not from the
HIP source.  Three parts: model_pack, model_parse, and a datagram builder that can produce what solo_rtp_pack never writes.

A session is a dict: n_streams, L (timestamp ticks per packet), level_id, and streams = {stream: dict(ssrc, ts_offset, seq_offset,
pt=(pt_md1, pt_md2))} for the bound streams."""
import struct

import numpy as np

INT32_MAX = 2 ** 31 - 1
VERDICTS = ("accepted", "malformed", "version", "unknown_ssrc", "unknown_pt", "timestamp")
REJECTED = (-1, 0, 0, 0, 0)


def session(n_streams, L, level_id=0, streams=None):
    return dict(n_streams=n_streams, L=L, level_id=level_id, streams=dict(streams or {}))


# ---- the builder ----------------------------------------------------------------------------------------------------------------------
def one_byte_elements(elements):
    """[(id, data bytes)] -> the elements of RFC 8285 section 4.2 back to back; id 0 with data b"" is ONE pad byte, id 15 is written as it is
    (a data length of 1 .. 16 bytes is what the form can express)"""
    out = b""
    for ident, data in elements:
        if ident == 0:
            out += b"\x00"
        else:
            assert 1 <= len(data) <= 16
            out += bytes([(ident << 4) | (len(data) - 1)]) + bytes(data)
    return out


def extension_block(profile, body, length_words=None):
    """the header extension of RFC 3550 section 5.3.1: profile, length in 32-bit words (of the body, padded with zeros -- or a value of the
    caller's that says something else), body"""
    body = bytes(body)
    body += b"\x00" * (-len(body) % 4)
    return struct.pack(">HH", profile, len(body) // 4 if length_words is None else length_words) + body


def build(ssrc, pt, seq16, ts, payload, version=2, csrc=(), pad=0, ext=None, x=None, marker=0, pad_count=None):
    """One datagram.  csrc: up to 15 contributing sources; pad: padding octets at the end (the last one holds the count -- or pad_count,
    where the caller wants it wrong; pad = 0 with pad_count given sets the P bit on an unpadded datagram, whose last PAYLOAD byte is then
    read as the count); ext: an extension_block() (sets X) or None; x: force the X bit without a block (or clear it with one)."""
    has_x = (ext is not None) if x is None else bool(x)
    has_p = pad > 0 or pad_count is not None
    b0 = (version << 6) | (has_p << 5) | (has_x << 4) | len(csrc)
    out = struct.pack(">BBHII", b0, (marker << 7) | pt, seq16 & 0xFFFF, ts & 0xFFFFFFFF, ssrc & 0xFFFFFFFF)
    for c in csrc:
        out += struct.pack(">I", c)
    if ext is not None:
        out += ext
    out += bytes(payload)
    if pad > 0:
        out += b"\x00" * (pad - 1) + bytes([pad if pad_count is None else pad_count])
    elif pad_count is not None and len(out) > 0:
        out = out[:-1] + bytes([pad_count])
    return out


def level_ext(level_id, level_byte):
    """what solo_rtp_pack writes behind the header: 0xBEDE, one word, the RFC 6464 element, two pad bytes"""
    return extension_block(0xBEDE, one_byte_elements([(level_id, bytes([level_byte]))]))


# ---- pack -----------------------------------------------------------------------------------------------------------------------------
def model_pack(ses, records, n_records, payload, level=None, max_records=None, cap=None):
    """records int32 [*,5] (stream, seq, desc, offset, len), n_records: what the sender's count says (< 0: a refused list), payload uint8,
    level uint8 [n_streams, depth] or None -> dict(dgrams [n,2], wire (the bytes written: a prefix of the full wire), count, all_dgrams,
    all_wire (without the cap), reasons)"""
    records = np.asarray(records)
    max_records = records.shape[0] if max_records is None else max_records
    if n_records < 0:
        return dict(count=dict(dgrams=-1), refused_list=True)
    n = min(n_records, max_records)
    cap = INT32_MAX if cap is None else min(cap, INT32_MAX)
    pool = bytes(np.asarray(payload, np.uint8))
    full, dg_full, reasons = bytearray(), [], {}
    for k in range(n):
        stream, seq, desc, off, ln = (int(v) for v in records[k])
        why = None
        if not 0 <= stream < ses["n_streams"]:
            why = "stream"
        elif stream not in ses["streams"]:
            why = "unbound"
        elif desc not in (0, 1):
            why = "desc"
        elif seq < 0:
            why = "seq"
        elif ln <= 0:
            why = "len"
        elif ln > 32767:
            why = "long"
        elif off < 0 or off + ln > len(pool):
            why = "range"
        if why:
            reasons[why] = reasons.get(why, 0) + 1
            dg_full.append(None)
            continue
        s = ses["streams"][stream]
        ext = None
        if level is not None:
            ext = level_ext(ses["level_id"], int(level[stream, seq % level.shape[1]]))
        d = build(s["ssrc"], s["pt"][desc], (s["seq_offset"] + 2 * seq + desc) % 65536, (s["ts_offset"] + seq * ses["L"]) % 2 ** 32, pool[off:off + ln], ext=ext)
        assert len(d) == (12 if level is None else 20) + ln
        assert len(full) % 4 == 0
        dg_full.append((len(full), len(d)))
        full += d + b"\x00" * (-len(d) % 4)
    dgrams = np.zeros((n, 2), np.int32)
    written = nbytes = 0
    for k, d in enumerate(dg_full):
        if d is not None and d[0] + ((d[1] + 3) & ~3) <= cap:
            dgrams[k] = d
            written += 1
            nbytes = d[0] + ((d[1] + 3) & ~3)
    valid = [d for d in dg_full if d is not None]
    count = dict(dgrams=written, dgrams_needed=len(valid), bytes=nbytes, bytes_needed=len(full), refused=n - len(valid), reserved=0)
    all_dgrams = np.array([d if d is not None else (0, 0) for d in dg_full], np.int32).reshape(n, 2)
    return dict(dgrams=dgrams, wire=np.frombuffer(bytes(full[:nbytes]), np.uint8), count=count, all_dgrams=all_dgrams,
                all_wire=np.frombuffer(bytes(full), np.uint8), reasons=reasons)


# ---- parse ----------------------------------------------------------------------------------------------------------------------------
def find_level(block, level_id):
    """the walk over the one-byte elements of an extension body -> the level byte or 255"""
    at = 0
    while at < len(block):
        ident, ln = block[at] >> 4, (block[at] & 15) + 1
        if ident == 0:
            at += 1
            continue
        if ident == 15 or at + 1 + ln > len(block):
            break
        if ident == level_id and ln == 1:
            return block[at + 1]
        at += 1 + ln
    return 255


def parse_one(ses, play, off, ln, wire):
    """-> (verdict, arrival, level byte, raw sequence number)"""
    wire_bytes = min(len(wire), INT32_MAX)
    if ln < 12 or off < 0 or off + ln > wire_bytes:
        return "malformed", REJECTED, 255, 0
    d = bytes(wire[off:off + ln])
    b0, b1, seq16, ts, ssrc = struct.unpack(">BBHII", d[:12])
    hdr = 12 + 4 * (b0 & 15)
    if hdr > ln:
        return "malformed", REJECTED, 255, 0
    profile, block = None, b""
    if b0 & 0x10:
        if hdr + 4 > ln:
            return "malformed", REJECTED, 255, 0
        profile, words = struct.unpack(">HH", d[hdr:hdr + 4])
        if hdr + 4 + 4 * words > ln:
            return "malformed", REJECTED, 255, 0
        block = d[hdr + 4:hdr + 4 + 4 * words]
        hdr += 4 + 4 * words
    pad = 0
    if b0 & 0x20:
        pad = d[-1]
        if pad == 0 or pad > ln - hdr:
            return "malformed", REJECTED, 255, 0
    n = ln - hdr - pad
    if n <= 0 or n > 32767:
        return "malformed", REJECTED, 255, 0
    if b0 >> 6 != 2:
        return "version", REJECTED, 255, 0
    stream = [s for s, c in ses["streams"].items() if c["ssrc"] == ssrc]
    if not stream:
        return "unknown_ssrc", REJECTED, 255, 0
    stream, = stream
    c = ses["streams"][stream]
    pt = b1 & 127
    if pt not in c["pt"]:
        return "unknown_pt", REJECTED, 255, 0
    desc = -1 if c["pt"][0] == c["pt"][1] else c["pt"].index(pt)
    L, p = ses["L"], int(play[stream])
    delta = (ts - c["ts_offset"] - p * L) % 2 ** 32
    if delta >= 2 ** 31:
        delta -= 2 ** 32
    if delta % L:
        return "timestamp", REJECTED, 255, 0
    seq = p + delta // L
    if not 0 <= seq <= INT32_MAX:
        return "timestamp", REJECTED, 255, 0
    level = 255
    if profile == 0xBEDE and ses["level_id"] > 0:
        level = find_level(block, ses["level_id"])
    return "accepted", (stream, seq, desc, off + hdr, n), level, seq16


def model_parse(ses, play, dgrams, wire):
    """dgrams int32 [n,2], wire uint8 -> dict(arrivals int32 [n,5], level uint8 [n], rtp_seq uint16 [n], count, verdicts)"""
    dgrams = np.asarray(dgrams).reshape(-1, 2)
    n = dgrams.shape[0]
    arrivals, level, rtp_seq = np.zeros((n, 5), np.int32), np.zeros(n, np.uint8), np.zeros(n, np.uint16)
    count = dict.fromkeys(("accepted", "with_level") + VERDICTS[1:] + ("reserved",), 0)
    verdicts = []
    w = np.asarray(wire, np.uint8)
    for i in range(n):
        v, a, lv, sq = parse_one(ses, play, int(dgrams[i, 0]), int(dgrams[i, 1]), w)
        arrivals[i], level[i], rtp_seq[i] = a, lv, sq
        count[v] += 1
        count["with_level"] += v == "accepted" and lv != 255
        verdicts.append(v)
    return dict(arrivals=arrivals, level=level, rtp_seq=rtp_seq, count=count, verdicts=verdicts)


# ---- inputs both test files share ------------------------------------------------------------------------------------------------------
def random_session(rng, n_streams, L, level_id, unbound=(), equal_pt=()):
    """every stream but `unbound` bound: distinct SSRCs (and distinct from each other's ^ 0x5A5A5A5A, which hostile_kinds uses as an unknown
    one), random offsets, payload types 96 / 97 (`equal_pt`: 98 / 98)"""
    ssrcs = set()
    while len(ssrcs) < n_streams:
        v = int(rng.integers(0, 2 ** 32))
        if v not in ssrcs and (v ^ 0x5A5A5A5A) not in ssrcs and not any((u ^ 0x5A5A5A5A) == v for u in ssrcs):
            ssrcs.add(v)
    ssrcs = sorted(ssrcs)
    rng.shuffle(ssrcs)
    streams = {s: dict(ssrc=int(ssrcs[s]), ts_offset=int(rng.integers(0, 2 ** 32)), seq_offset=int(rng.integers(0, 2 ** 16)),
                       pt=(98, 98) if s in equal_pt else (96, 97)) for s in range(n_streams) if s not in unbound}
    return session(n_streams, L, level_id, streams)


def random_records(rng, ses, n, pool_bytes, seq_lo=0, seq_hi=1000, hostile=True, max_len=120):
    """n records over a pool of pool_bytes: lengths 1 .. max_len, offsets that repeat (a tenth of the records share another's), and with
    `hostile` every refusal reason mixed in"""
    N = ses["n_streams"]
    rec = np.zeros((n, 5), np.int64)
    rec[:, 0] = rng.integers(0, N, n)
    rec[:, 1] = rng.integers(seq_lo, seq_hi, n)
    rec[:, 2] = rng.integers(0, 2, n)
    rec[:, 4] = rng.integers(1, max_len + 1, n)
    rec[:, 3] = (rng.random(n) * (pool_bytes - rec[:, 4] + 1)).astype(np.int64)
    share = np.nonzero(rng.random(n) < 0.1)[0]
    src = rng.integers(0, n, share.size)
    rec[share, 3], rec[share, 4] = rec[src, 3], rec[src, 4]
    if hostile:
        kind = rng.random(n)
        for lo, col, values in ((0.00, 0, (-1, N, N + 7, -2 ** 31)), (0.03, 2, (-1, 2, 3)), (0.06, 1, (-1, -2 ** 31)), (0.09, 4, (0, -5)),
                                (0.12, 4, (32768, 40000, INT32_MAX)), (0.15, 3, (-1, pool_bytes, INT32_MAX))):
            m = np.nonzero((kind >= lo) & (kind < lo + 0.03))[0]
            rec[m, col] = rng.choice(values, m.size)
        m = np.nonzero((kind >= 0.18) & (kind < 0.21))[0]                   # ends one byte behind the pool
        rec[m, 3] = pool_bytes - rec[m, 4] + 1
        m = np.nonzero((kind >= 0.21) & (kind < 0.23))[0]                   # ends with the pool: valid
        rec[m, 3] = pool_bytes - rec[m, 4]
    return rec.astype(np.int32)


# ---- hostile datagrams: every kind solo_rtp_pack never writes, each with the verdict it must get --------------------------------------
def hostile_kinds(ses, play, stream, rng):
    """-> [(name, datagram bytes, expected verdict, expected level or None)] for a bound stream of the session with distinct payload types
    and a level_id > 0; timestamps are the stream's play-out position plus 0 .. 3 packets"""
    c, L, lid = ses["streams"][stream], ses["L"], ses["level_id"]
    assert lid > 0 and c["pt"][0] != c["pt"][1]
    other = lid % 14 + 1

    def ts():
        return c["ts_offset"] + (int(play[stream]) + int(rng.integers(0, 4))) * L

    def pl(n=None):
        return rng.integers(0, 256, int(rng.integers(1, 60)) if n is None else n, dtype=np.uint8).tobytes()

    def el(*e):
        return extension_block(0xBEDE, one_byte_elements(list(e)))

    A, M = "accepted", "malformed"
    kinds = [
        ("plain", build(c["ssrc"], c["pt"][0], 7, ts(), pl()), A, 255),
        ("md2", build(c["ssrc"], c["pt"][1], 8, ts(), pl()), A, 255),
        ("marker", build(c["ssrc"], c["pt"][0], 9, ts(), pl(), marker=1), A, 255),
        ("cc1", build(c["ssrc"], c["pt"][0], 10, ts(), pl(), csrc=[5]), A, 255),
        ("cc15", build(c["ssrc"], c["pt"][1], 11, ts(), pl(), csrc=list(range(15))), A, 255),
        ("cc15_level", build(c["ssrc"], c["pt"][1], 11, ts(), pl(), csrc=list(range(15)), ext=level_ext(lid, 0x85)), A, 0x85),
        ("padding", build(c["ssrc"], c["pt"][0], 12, ts(), pl(), pad=3), A, 255),
        ("padding_all", build(c["ssrc"], c["pt"][0], 12, ts(), b"", pad=5), M, None),
        ("padding_zero", build(c["ssrc"], c["pt"][0], 12, ts(), pl(9), pad_count=0), M, None),
        ("padding_over", build(c["ssrc"], c["pt"][0], 12, ts(), pl(9), pad=4, pad_count=14), M, None),
        ("padding_max", build(c["ssrc"], c["pt"][0], 12, ts(), pl(1), pad=255), A, 255),
        ("level", build(c["ssrc"], c["pt"][0], 13, ts(), pl(), ext=level_ext(lid, 0x9C)), A, 0x9C),
        ("level_after_others", build(c["ssrc"], c["pt"][0], 14, ts(), pl(), ext=el((other, b"abc"), (0, b""), (0, b""), (lid, b"\x2A"), (other, b"z"))), A, 0x2A),
        ("level_len2", build(c["ssrc"], c["pt"][0], 15, ts(), pl(), ext=el((lid, b"\x11\x22"))), A, 255),
        ("level_len2_then_1", build(c["ssrc"], c["pt"][0], 15, ts(), pl(), ext=el((lid, b"\x11\x22"), (lid, b"\x33"))), A, 0x33),
        ("level_behind_15", build(c["ssrc"], c["pt"][0], 16, ts(), pl(), ext=extension_block(0xBEDE, b"\xF0" + one_byte_elements([(lid, b"\x44")]))), A, 255),
        ("overrun", build(c["ssrc"], c["pt"][0], 17, ts(), pl(), ext=extension_block(0xBEDE, bytes([(other << 4) | 7, 1, 2, 3, lid << 4, 0x55, 0, 0]))), A, 255),
        ("overrun_level", build(c["ssrc"], c["pt"][0], 17, ts(), pl(), ext=extension_block(0xBEDE, b"\x00\x00\x00" + bytes([lid << 4]))), A, 255),
        ("other_profile", build(c["ssrc"], c["pt"][0], 18, ts(), pl(), ext=extension_block(0x1000, one_byte_elements([(lid, b"\x66")]))), A, 255),
        ("two_byte_form", build(c["ssrc"], c["pt"][0], 18, ts(), pl(), ext=extension_block(0x1000, bytes([lid, 1, 0x66, 0]))), A, 255),
        ("empty_ext", build(c["ssrc"], c["pt"][0], 19, ts(), pl(), ext=extension_block(0xBEDE, b"")), A, 255),
        ("x_no_room", build(c["ssrc"], c["pt"][0], 20, ts(), b"", x=True), M, None),
        ("x_short_room", build(c["ssrc"], c["pt"][0], 20, ts(), pl(3), x=True), M, None),
        ("x_block_past_end", build(c["ssrc"], c["pt"][0], 20, ts(), pl(5), ext=extension_block(0xBEDE, b"", length_words=9)), M, None),
        ("x_block_eats_payload", build(c["ssrc"], c["pt"][0], 20, ts(), b"", ext=level_ext(lid, 1)), M, None),
        ("cc_past_end", build(c["ssrc"], c["pt"][0], 21, ts(), pl(4), csrc=[1, 2])[:16], M, None),
        ("version1", build(c["ssrc"], c["pt"][0], 22, ts(), pl(), version=1), "version", None),
        ("version3", build(c["ssrc"], c["pt"][0], 22, ts(), pl(), version=3), "version", None),
        ("version0_and_cc_past_end", build(c["ssrc"], c["pt"][0], 22, ts(), pl(2), version=0, csrc=[1, 2, 3])[:18], M, None),      # two rules: the earlier one
        ("version1_unknown_ssrc", build(c["ssrc"] ^ 0x5A5A5A5A, c["pt"][0], 22, ts(), pl(), version=1), "version", None),           # two rules
        ("truncated_11", build(c["ssrc"], c["pt"][0], 23, ts(), b"")[:11], M, None),
        ("truncated_1", build(c["ssrc"], c["pt"][0], 23, ts(), b"")[:1], M, None),
        ("zero_payload", build(c["ssrc"], c["pt"][0], 24, ts(), b""), M, None),
        ("unknown_ssrc", build(c["ssrc"] ^ 0x5A5A5A5A, c["pt"][0], 25, ts(), pl()), "unknown_ssrc", None),
        ("unknown_ssrc_and_pt", build(c["ssrc"] ^ 0x5A5A5A5A, (max(c["pt"]) + 1) % 128, 25, ts(), pl()), "unknown_ssrc", None),    # two rules
        ("unknown_pt", build(c["ssrc"], (max(c["pt"]) + 1) % 128, 26, ts(), pl()), "unknown_pt", None),
        ("unknown_pt_bad_ts", build(c["ssrc"], (max(c["pt"]) + 1) % 128, 26, ts() + 1, pl()), "unknown_pt", None),                  # two rules
        ("ts_off_grid", build(c["ssrc"], c["pt"][0], 27, ts() + 1, pl()), "timestamp", None),
        ("ts_off_grid_level", build(c["ssrc"], c["pt"][0], 27, ts() + L - 1, pl(), ext=level_ext(lid, 3)), "timestamp", None),
    ]
    return kinds

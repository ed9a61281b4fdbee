"""An independent model of the RTCP calls (solo_rtcp_*, include/solo_mi355x.h) in plain Python integers, written from RFC 3550 section
6.4 and its appendix A.1 (update_seq), A.2 (validity of a compound packet), A.3 (loss), A.8 (jitter): one datagram at a time, in index
order.  It shares no code with the product.  It also holds a byte-level writer and reader of SR / RR / SDES / BYE, the scenarios that the
CPU suite (tests/test_rtcp_model.py) and the GPU suite (tests/test_gpu_rtcp.py) both run, and the driver that compares an implementation
with the model after every tick."""
import random
import struct

import numpy as np

M32 = 0xFFFFFFFF
RTP_SEQ_MOD = 1 << 16
MAX_DROPOUT = 3000
MAX_MISORDER = 100
WORDS = 32
CNAME_BYTES = 32
FIELDS = ("base_seq", "max_seq", "cycles", "bad_seq", "received", "expected_prior", "received_prior", "transit", "jitter", "seen", "lsr",
          "lsr_arrival", "tx_packets", "tx_octets", "tx_next", "tx_since")
RECEIVED_COUNT = ("counted", "first", "in_order", "misordered", "dropout_pending", "resynced", "not_counted")
SENT_COUNT = ("sent", "skipped")
BUILD_COUNT = ("built", "built_needed", "bytes", "bytes_needed", "refused", "with_sr")
PARSE_COUNT = ("accepted", "malformed", "version", "first_type", "length", "sr", "blocks", "unknown_ssrc", "bye", "skipped")
FEEDBACK = ("seen", "fraction_lost", "cum_lost", "ext_high_seq", "jitter", "lsr", "dlsr", "rtt")
BYE_BIT = 1 << 30
SEEN, HAS_TRANSIT, HAS_SR = 1, 2, 4


def mid32(ntp):
    return (ntp >> 16) & M32


def s32(v):
    v &= M32
    return v - (1 << 32) if v & 0x80000000 else v


# ---- the wire: writer and reader ----------------------------------------------------------------------------------------------------
def write_block(ssrc, fraction, lost, ext_seq, jitter, lsr, dlsr):
    return struct.pack(">IIIIII", ssrc, ((fraction & 255) << 24) | (lost & 0xFFFFFF), ext_seq & M32, jitter & M32, lsr & M32, dlsr & M32)


def write_sr(ssrc, ntp, rtp_ts, packets, octets, blocks=()):
    body = struct.pack(">IIIIII", ssrc, (ntp >> 32) & M32, ntp & M32, rtp_ts & M32, packets & M32, octets & M32) + b"".join(blocks)
    return struct.pack(">BBH", 0x80 | len(blocks), 200, len(body) // 4) + body


def write_rr(ssrc, blocks=()):
    body = struct.pack(">I", ssrc) + b"".join(blocks)
    return struct.pack(">BBH", 0x80 | len(blocks), 201, len(body) // 4) + body


def write_sdes(ssrc, cname):
    body = struct.pack(">I", ssrc) + bytes([1, len(cname)]) + cname + b"\0"
    body += b"\0" * (-len(body) % 4)
    return struct.pack(">BBH", 0x81, 202, len(body) // 4) + body


def write_bye(ssrcs):
    body = b"".join(struct.pack(">I", x) for x in ssrcs)
    return struct.pack(">BBH", 0x80 | len(ssrcs), 203, len(body) // 4) + body


def read_compound(data):
    """-> (verdict, packets): verdict "accepted" or the first rule of A.2 that fails; packets = [(pt, count, body without padding)]"""
    n = len(data)
    if n < 4:
        return "malformed", []
    if data[0] >> 6 != 2:
        return "version", []
    if (data[0] >> 5) & 1 or data[1] not in (200, 201):
        return "first_type", []
    at, out = 0, []
    while at < n:
        if at + 4 > n:
            return "length", []
        b0, pt, words = struct.unpack_from(">BBH", data, at)
        if b0 >> 6 != 2:
            return "version", []
        plen = 4 * (words + 1)
        if at + plen > n:
            return "length", []
        body = data[at + 4:at + plen]
        if (b0 >> 5) & 1:
            pad = data[n - 1]
            if at + plen != n or pad == 0 or pad % 4 or pad > len(body):
                return "length", []
            body = body[:len(body) - pad]
        rc = b0 & 31
        need = {200: 24 + 24 * rc, 201: 4 + 24 * rc, 203: 4 * rc}.get(pt, 0)
        if len(body) < need:
            return "length", []
        out.append((pt, rc, body))
        at += plen
    return "accepted", out


# ---- the model ------------------------------------------------------------------------------------------------------------------------
class Session:
    """what the calls read of an RTP session: per stream an SSRC, a timestamp offset and whether it is bound"""

    def __init__(self, ssrc, ts_offset, bound=None, packet_samples=640):
        self.ssrc, self.ts_offset = [int(x) for x in ssrc], [int(x) for x in ts_offset]
        self.bound = [1] * len(self.ssrc) if bound is None else [int(x) for x in bound]
        self.L = packet_samples
        self.n = len(self.ssrc)

    def find(self, ssrc):
        for s in range(self.n):
            if self.bound[s] and self.ssrc[s] == ssrc:
                return s
        return -1

    def cfg(self):
        """uint32 [n][4] as the device holds it: {ssrc, ts_offset, seq_pt, bound} (an unbound record is zero)"""
        c = np.zeros((self.n, 4), np.uint32)
        for s in range(self.n):
            if self.bound[s]:
                c[s] = (self.ssrc[s], self.ts_offset[s], (96 << 16) | (97 << 24), 1)
        return c


class Model:
    def __init__(self, n):
        self.n = n
        self.rows = [dict.fromkeys(FIELDS, 0) for _ in range(n)]
        self.cname = [b""] * n

    def reset_rows(self, rows):
        for s in rows:
            self.rows[s] = dict.fromkeys(FIELDS, 0)
            self.cname[s] = b""

    def set_cname(self, streams, names):
        for s, c in zip(streams, names):
            self.cname[s] = bytes(c)

    def words(self):
        """uint32 [n][40]: the state blob"""
        w = np.zeros((self.n, WORDS + CNAME_BYTES // 4), np.uint32)
        for s, r in enumerate(self.rows):
            w[s, :len(FIELDS)] = [r[f] & M32 for f in FIELDS]
            w[s, WORDS:] = np.frombuffer(self.cname[s].ljust(CNAME_BYTES, b"\0"), "<u4")
        return w

    def set_words(self, w):
        for s, r in enumerate(self.rows):
            for k, f in enumerate(FIELDS):
                r[f] = int(w[s, k])
            self.cname[s] = w[s, WORDS:].astype("<u4").tobytes().split(b"\0")[0]

    # A.1, without probation
    @staticmethod
    def _init_seq(r, seq):
        r["base_seq"] = r["max_seq"] = seq
        r["bad_seq"] = RTP_SEQ_MOD + 1
        r["cycles"] = r["received"] = r["received_prior"] = r["expected_prior"] = 0

    def _update_seq(self, r, seq):
        if not r["seen"] & SEEN:
            self._init_seq(r, seq)
            r["seen"] |= SEEN
            out = "first"
        else:
            udelta = (seq - r["max_seq"]) % RTP_SEQ_MOD
            if udelta < MAX_DROPOUT:
                if seq < r["max_seq"]:
                    r["cycles"] = (r["cycles"] + RTP_SEQ_MOD) & M32
                r["max_seq"] = seq
                out = "in_order"
            elif udelta <= RTP_SEQ_MOD - MAX_MISORDER:
                if seq == r["bad_seq"]:
                    self._init_seq(r, seq)
                    out = "resynced"
                else:
                    r["bad_seq"] = (seq + 1) & (RTP_SEQ_MOD - 1)
                    return "dropout_pending", False
            else:
                out = "misordered"
        r["received"] = (r["received"] + 1) & M32
        return out, True

    def received(self, session, arrivals, rtp_seq, arrival_time, now_rtp):
        c = dict.fromkeys(RECEIVED_COUNT, 0)
        for i in range(len(arrivals)):
            s, q = int(arrivals[i][0]), int(arrivals[i][1])
            if not 0 <= s < self.n:
                c["not_counted"] += 1
                continue
            r = self.rows[s]
            out, accepted = self._update_seq(r, int(rtp_seq[i]) & 0xFFFF)
            c[out] += 1
            c["counted"] += 1
            if accepted:                                        # A.8
                arrival = int(arrival_time[i]) & M32 if arrival_time is not None else now_rtp
                transit = (arrival - (session.ts_offset[s] + q * session.L)) & M32
                if r["seen"] & HAS_TRANSIT:
                    d = abs(s32(transit - r["transit"]))
                    r["jitter"] = (r["jitter"] + d - ((r["jitter"] + 8) >> 4)) & M32
                r["transit"] = transit
                r["seen"] |= HAS_TRANSIT
        return c

    def sent(self, records, n_records, dgrams):
        c = dict.fromkeys(SENT_COUNT, 0)
        if n_records < 0:
            c["sent"] = -1
            return c
        for k in range(min(n_records, len(records))):
            s, q, _, _, ln = (int(v) for v in records[k])
            if int(dgrams[k][1]) <= 0 or not 0 <= s < self.n:
                c["skipped"] += 1
                continue
            r = self.rows[s]
            r["tx_packets"] = (r["tx_packets"] + 1) & M32
            r["tx_octets"] = (r["tx_octets"] + ln) & M32
            r["tx_since"] = (r["tx_since"] + 1) & M32
            r["tx_next"] = max(r["tx_next"], (q + 1) & M32)
            c["sent"] += 1
        return c

    def report_block(self, s, ssrc, now):
        """A.3 -> (the block's bytes, expected)"""
        r = self.rows[s]
        expected = (r["cycles"] + r["max_seq"] - r["base_seq"] + 1) & M32
        lost = max(-0x800000, min(0x7FFFFF, s32(expected - r["received"])))
        expected_interval = (expected - r["expected_prior"]) & M32
        received_interval = (r["received"] - r["received_prior"]) & M32
        lost_interval = s32(expected_interval - received_interval)
        fraction = 0 if expected_interval == 0 or lost_interval <= 0 else min(255, (lost_interval << 8) // expected_interval)
        has_sr = r["seen"] & HAS_SR
        return write_block(ssrc, fraction, lost, r["cycles"] | r["max_seq"], r["jitter"] >> 4, r["lsr"] if has_sr else 0,
                           (mid32(now) - r["lsr_arrival"]) & M32 if has_sr else 0), expected

    def build(self, tx, rx, streams, now, cap):
        """-> (refused call?, dgrams [(offset, len)], wire bytes, count)"""
        c = dict.fromkeys(BUILD_COUNT, 0)
        if any(not 0 <= s < self.n for s in streams) or any(b <= a for a, b in zip(streams, streams[1:])):
            c["built"] = -1
            return True, [], b"", c
        cap = min(cap, 0x7FFFFFFF)
        dgrams, wire, off = [], bytearray(), 0
        for s in streams:
            if not tx.bound[s] or not self.cname[s]:
                c["refused"] += 1
                dgrams.append((0, 0))
                continue
            r = self.rows[s]
            blocks, expected = [], None
            if rx is not None and rx.bound[s] and r["seen"] & SEEN:
                blk, expected = self.report_block(s, rx.ssrc[s], now)
                blocks.append(blk)
            sr = r["tx_since"] > 0
            if sr:
                pkt = write_sr(tx.ssrc[s], now, tx.ts_offset[s] + r["tx_next"] * tx.L, r["tx_packets"], r["tx_octets"], blocks)
            else:
                pkt = write_rr(tx.ssrc[s], blocks)
            pkt += write_sdes(tx.ssrc[s], self.cname[s])
            c["built_needed"] += 1
            c["bytes_needed"] += len(pkt)
            if off + len(pkt) <= cap:
                assert len(wire) == off
                wire += pkt
                dgrams.append((off, len(pkt)))
                c["built"] += 1
                c["bytes"] += len(pkt)
                c["with_sr"] += sr
                if expected is not None:
                    r["expected_prior"], r["received_prior"] = expected, r["received"]
                r["tx_since"] = 0
            else:
                dgrams.append((0, 0))
            off += len(pkt)
        return False, dgrams, bytes(wire), c

    def parse(self, rx, tx, dgrams, wire, now):
        """-> (feedback: one dict per stream, count)"""
        c = dict.fromkeys(PARSE_COUNT, 0)
        fb = [dict(dict.fromkeys(FEEDBACK, 0), rtt=-1) for _ in range(self.n)]
        for off, ln in dgrams:
            off, ln = int(off), int(ln)
            if ln < 4 or off < 0 or off + ln > min(len(wire), 0x7FFFFFFF):
                c["malformed"] += 1
                continue
            verdict, packets = read_compound(bytes(wire[off:off + ln]))
            c[verdict] += 1
            for pt, rc, body in packets:
                if pt in (200, 201):
                    at = 4
                    if pt == 200:
                        ssrc, hi, lo = struct.unpack_from(">III", body, 0)
                        s = rx.find(ssrc)
                        if s < 0:
                            c["unknown_ssrc"] += 1
                        else:
                            c["sr"] += 1
                            r = self.rows[s]
                            r["lsr"], r["lsr_arrival"] = mid32((hi << 32) | lo), mid32(now)
                            r["seen"] |= HAS_SR
                        at = 24
                    for b in range(rc):
                        ssrc, w1, ext, jit, lsr, dlsr = struct.unpack_from(">IIIIII", body, at + 24 * b)
                        s = tx.find(ssrc) if tx is not None else -1
                        if s < 0:
                            continue
                        c["blocks"] += 1
                        cum = w1 & 0xFFFFFF
                        rtt = -1 if lsr == 0 else max(0, s32(mid32(now) - lsr - dlsr))
                        fb[s].update(seen=(fb[s]["seen"] & ~BYE_BIT) + 1 | (fb[s]["seen"] & BYE_BIT), fraction_lost=w1 >> 24,
                                     cum_lost=cum - (1 << 24) if cum & 0x800000 else cum, ext_high_seq=ext, jitter=jit, lsr=lsr, dlsr=dlsr, rtt=rtt)
                elif pt == 203:
                    for b in range(rc):
                        s = rx.find(struct.unpack_from(">I", body, 4 * b)[0])
                        if s >= 0:
                            c["bye"] += 1
                            fb[s]["seen"] |= BYE_BIT
                else:
                    c["skipped"] += 1
        return fb, c


def feedback_array(fb):
    return np.array([[f[k] & M32 for k in FEEDBACK] for f in fb], np.uint32).reshape(-1, 8)


# ---- scenarios of received(): ticks of (arrivals int32 [n,5], rtp_seq uint16 [n], arrival_time uint32 [n] or None, now_rtp) ---------------
def interleave(rng, per_stream):
    """the streams' lists merged in a random order that keeps every stream's own order"""
    pos = [0] * len(per_stream)
    left = [s for s, l in enumerate(per_stream) for _ in l]
    rng.shuffle(left)
    out = []
    for s in left:
        out.append(per_stream[s][pos[s]])
        pos[s] += 1
    return out


def make_tick(items, with_time, now_rtp):
    """items: (stream, packet number, desc, rtp_seq, arrival time)"""
    n = len(items)
    arr = np.zeros((n, 5), np.int32)
    seq, at = np.zeros(n, np.uint16), np.zeros(n, np.uint32)
    for i, (s, q, d, sq, t) in enumerate(items):
        arr[i] = (s, q, d, 12 + 64 * i, 40 if s >= 0 else 0)
        seq[i], at[i] = sq & 0xFFFF, t & M32
    return dict(arrivals=arr, rtp_seq=seq, arrival_time=at if with_time else None, now_rtp=now_rtp & M32)


def scenario(name, n, ticks, seed, session, seq_offset, walk_max=128):
    """-> list of ticks.  (a) clean; (b) loss 20 %, reordering inside a call, duplicates; (c) as (a): the caller brings seq_offset = 65530
    and a clock that crosses 2^32; (d) jumps of 2999 / 3000 / 3001, resync, misorder of 99 / 100 / 101; (e) one stream with walk_max - 1,
    walk_max, walk_max + 1 and 300 datagrams in a call, an empty call, rejected arrivals, desc = -1"""
    rng = random.Random(seed)
    L = session.L
    clock = 0xFFFFFFFF - 5 * L if name == "c" else 1000
    out = []
    q = [0] * n                                              # next packet number per stream
    jump = [0] * n                                           # (d): what is added to the sequence numbers
    for t in range(ticks):
        per = [[] for _ in range(n)]
        for s in range(n):
            k, most = 2 if name == "c" else 1, None
            if name == "e" and s == 3 % n:
                most = {2: walk_max - 1, 4: walk_max, 6: walk_max + 1, 8: 300}.get(t)
                k = 1 if most is None else (most + 1) // 2
            for _ in range(k):
                for d in (0, 1):
                    sq = seq_offset[s] + 2 * q[s] + d + jump[s]
                    at = clock + session.ts_offset[s] + q[s] * L + rng.randrange(0, 200) + (37 * s) % 90
                    item = (s, q[s], -1 if name == "e" and s == 1 % n else d, sq, at)
                    if name == "b" and rng.random() < 0.2:
                        continue
                    per[s].append(item)
                    if name == "b" and rng.random() < 0.1:
                        per[s].append(item)
                q[s] += 1
            if most is not None:
                del per[s][most:]
            if name == "b" and len(per[s]) > 1 and rng.random() < 0.5:
                rng.shuffle(per[s])
            if name == "d":
                if t == 3 + s % 5:
                    jump[s] += (2999, 3000, 3001)[s % 3] - 1     # (the next datagram continues by 1 anyway)
                if t == 12 + s % 5 and per[s]:                  # a datagram from the past, in front of this tick's
                    back = (99, 100, 101)[s % 3] + 1                 # (a[3] is max_seq + 1)
                    a = per[s][0]
                    per[s].insert(0, (a[0], a[1], a[2], a[3] - back, a[4]))
        items = interleave(rng, per)
        if name == "e":
            if t == 5:
                items = []
            for k in range(len(items) // 7):
                items.insert(rng.randrange(len(items) + 1), (-1, 0, 0, 0, 0))
            if t == 7:
                items.append((n, 1, 0, 5, 5))                   # a stream index just outside
        out.append(make_tick(items, with_time=name != "a" or t % 2 == 0, now_rtp=clock + t * L))
    return out


def run_received(impl, model, session, ticks, check):
    """every tick through impl.received(session, tick) -> count dict and impl.words() -> uint32 [n][40], compared with the model"""
    for t, tick in enumerate(ticks):
        want = model.received(session, tick["arrivals"], tick["rtp_seq"], tick["arrival_time"], tick["now_rtp"])
        got = impl.received(session, tick)
        check(got == want, "tick %d: count %s, model %s" % (t, got, want))
        w, mw = impl.words(), model.words()
        bad = np.argwhere(w != mw)
        check(bad.size == 0, "tick %d: state differs at (row, word) %s: %s, model %s" % (t, bad[:4].tolist(), w[tuple(bad[0])] if bad.size else 0,
                                                                                       mw[tuple(bad[0])] if bad.size else 0))


# ---- drivers of sent / build / parse: the same steps through an implementation and the model, compared after every step ------------------
def same_state(impl, model, check, what):
    w, mw = impl.words(), model.words()
    bad = np.argwhere(w != mw)
    check(bad.size == 0, "%s: state differs at (row, word) %s" % (what, bad[:4].tolist()))


def both_build(impl, model, tx, rx, streams, now, cap, check, what, **kw):
    """one build call through both -> (dgrams, wire) of the model"""
    refused, md, mw, mc = model.build(tx, rx, list(streams), now, cap)
    r, d, w, c = impl.build(tx, rx, streams, now, cap, **kw)
    if refused:
        check(r == 1 and c["built"] == -1, "%s: a refused list, got %d %s" % (what, r, c))
    else:
        check(r == 0 and c == mc, "%s: count %s, model %s" % (what, c, mc))
        check([tuple(x) for x in d.tolist()] == md, "%s: dgrams %s, model %s" % (what, d.tolist()[:6], md[:6]))
        check(bytes(w[:len(mw)]) == mw, "%s: wire bytes differ" % what)
    same_state(impl, model, check, what)
    return md, mw


def both_parse(impl, model, rx, tx, dgrams, wire, now, check, what, **kw):
    mfb, mc = model.parse(rx, tx, dgrams, wire, now)
    fb, c = impl.parse(rx, tx, np.asarray(dgrams, np.int32).reshape(-1, 2), np.frombuffer(bytes(wire), np.uint8), now, **kw)
    check(c == mc, "%s: count %s, model %s" % (what, c, mc))
    check(np.array_equal(fb, feedback_array(mfb)), "%s: feedback differs: %s, model %s" % (what, fb[:3].tolist(), feedback_array(mfb)[:3].tolist()))
    same_state(impl, model, check, what)
    return mfb, mc


def random_records(rng, n, m, first_seq):
    """m records {stream, seq, desc, offset, len} and their datagrams: some refused by the packer (len 0), some outside the streams"""
    rec, dg = np.zeros((m, 5), np.int32), np.zeros((m, 2), np.int32)
    for k in range(m):
        s = rng.randrange(-1, n + 1)
        ln = rng.randrange(1, 300)
        rec[k] = (s, first_seq + rng.randrange(0, 50), rng.randrange(2), 16 * k, ln)
        dg[k] = (400 * k, 0 if rng.random() < 0.15 else 12 + ln)
    return rec, dg


def run_sent_build(impl, model, tx, rx, check, seed=5, ticks=12):
    """records of random streams through sent(), then build() for changing lists and caps"""
    rng = random.Random(seed)
    n = model.n
    for t in range(ticks):
        m = rng.randrange(1, 3 * n + 2)
        rec, dg = random_records(rng, n, m, 40 * t)
        n_rec = -1 if t == 7 else rng.choice((m, m, max(1, m // 2), m + 3))
        want = model.sent(rec, min(n_rec, m), dg)
        got = impl.sent(tx, rec, n_rec, dg)
        check(got == want, "sent, tick %d: %s, model %s" % (t, got, want))
        same_state(impl, model, check, "sent, tick %d" % t)
        if t % 3 == 2:
            streams = sorted(rng.sample(range(n), rng.randrange(1, n + 1)))
            need = model_bytes_needed(model, tx, rx, streams, t)
            cap = {2: 1 << 40, 5: 0, 8: max(0, need - 1), 11: need}.get(t, 1 << 20)
            both_build(impl, model, tx, rx if t % 2 else None, streams, (0x83AA7E80 + t << 32) | 0x12345678, cap, check, "build, tick %d" % t)
    both_build(impl, model, tx, rx, [1, 1], 5, 1 << 20, check, "a list with a stream twice")
    both_build(impl, model, tx, rx, [0, n], 5, 1 << 20, check, "a list with a stream outside")
    both_build(impl, model, tx, rx, [2, 1], 5, 1 << 20, check, "a list that is not increasing")


def model_bytes_needed(model, tx, rx, streams, t):
    import copy
    m = copy.deepcopy(model)
    return m.build(tx, rx if t % 2 else None, list(streams), 0, 1 << 40)[3]["bytes_needed"]


def run_loopback(A, mA, B, mB, X, Y, check, d_units=3 << 24, net=5 << 20, now_kw=None):
    """side A (sends as X, hears Y) builds; side B (sends as Y, hears X) parses, then builds d_units later; A parses: the round-trip time
    is the two network delays exactly.  Then the rules of the index order and of rejected packets.  All times in units of 2^-32 s and
    multiples of 2^16, so the middle 32 bits subtract exactly"""
    kw = now_kw or {}
    n = mA.n
    streams = list(range(n))
    now0 = (0x83AA7E80 << 32) | (0x4000 << 16)
    dA, wA = both_build(A, mA, X, Y, streams, now0, 1 << 20, check, "A builds", **kw)
    both_parse(B, mB, X, Y, dA, wA, now0 + net, check, "B parses", **kw)
    now1 = now0 + net + d_units
    dB, wB = both_build(B, mB, Y, X, streams, now1, 1 << 20, check, "B builds", **kw)
    fb, c = both_parse(A, mA, Y, X, dB, wB, now1 + net, check, "A parses", **kw)
    for s in range(n):
        if fb[s]["seen"]:
            check(fb[s]["rtt"] == mid32(2 * net) and fb[s]["dlsr"] == mid32(d_units), "stream %d: rtt %d dlsr %d" % (s, fb[s]["rtt"], fb[s]["dlsr"]))
    check(c["blocks"] > 0 and c["sr"] > 0, "the loopback carried SRs and blocks: %s" % c)
    # two SRs of one stream in one call: the one in the higher datagram index wins, wherever its stamp lies
    old, new = write_sr(Y.ssrc[0], now0 - (9 << 32), 1, 2, 3), write_sr(Y.ssrc[0], now1, 4, 5, 6)
    for order in ((new, old), (old, new)):
        wire = order[0] + order[1]
        both_parse(A, mA, Y, X, [(0, len(order[0])), (len(order[0]), len(order[1]))], wire, now1 + 2 * net, check, "two SRs", **kw)
        check(mA.rows[0]["lsr"] == mid32(now0 - (9 << 32) if order[1] is old else now1), "the later index wins")
    # BYE; then what must be rejected with every state word unchanged
    rr = write_rr(Y.ssrc[1])
    good = rr + write_sdes(Y.ssrc[1], b"x") + write_bye([Y.ssrc[1], 0xDEAD0001, Y.ssrc[2 % n]])
    both_parse(A, mA, Y, X, [(0, len(good))], good, now1, check, "BYE", **kw)
    before = mA.words().copy()
    sr = write_sr(Y.ssrc[0], now1 + 77, 1, 2, 3, [write_block(X.ssrc[0], 1, 2, 3, 4, 5, 6)])
    inner = bytearray(sr + write_sdes(Y.ssrc[0], b"abc"))
    inner[len(sr) + 3] += 1                                 # the SDES claims one word more: the walk no longer ends at the end
    padded = bytearray(rr + write_sdes(Y.ssrc[1], b"x") + b"\0\0\0\4")
    padded[len(rr)] |= 0x20
    padded[len(rr) + 3] += 1
    cases = [("SDES first", write_sdes(Y.ssrc[0], b"abc") + sr, "first_type"), ("truncated", (sr + write_sdes(Y.ssrc[0], b"abc"))[:-4], "length"),
             ("inner length", bytes(inner), "length"), ("version", bytes([0x40]) + sr[1:], "version"), ("inner version", rr + bytes([0x01]) + sr[1:], "version"),
             ("padding on the first", bytes([sr[0] | 0x20]) + sr[1:], "first_type"), ("short", b"\x80\xc9", "malformed"),
             ("blocks beyond the packet", bytes([0x82]) + rr[1:], "length")]
    for what, data, verdict in cases:
        _, c = both_parse(A, mA, Y, X, [(0, len(data))], data, now1 + 99, check, what, **kw)
        check(c[verdict] == 1 and c["accepted"] == 0, "%s: %s" % (what, c))
        check(np.array_equal(mA.words(), before), "%s changed the state" % what)
    _, c = both_parse(A, mA, Y, X, [(0, len(padded))], bytes(padded), now1, check, "padding on the last", **kw)
    check(c["accepted"] == 1, "padding on the last packet is allowed: %s" % c)
    _, c = both_parse(A, mA, Y, X, [(-4, 8), (len(good) - 4, 8), (0, len(good))], good, now1, check, "ranges", **kw)
    check(c["malformed"] == 2 and c["accepted"] == 1, "ranges outside the wire: %s" % c)

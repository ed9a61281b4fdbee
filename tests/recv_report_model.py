"""Independent model of the receiver ring and of its read side (solo_recv_track, solo_recv_report), written from the definitions of the
interface and not from the kernels: a stream's queue is a dict {sequence number: [bytes of MD1, bytes of MD2 || HB]} -- there is no ring,
no length word and no rotation in here.  Filing follows tests/test_recv_ring.py::_model_file.  Used by the CPU comparison with the host
build of solo_recv_report.h (tests/test_recv_report_model.py) and by the play-out simulation on the GPU (tests/test_gpu_recv_report.py)."""
import numpy as np

INSERTED, LATE, AHEAD, DUP, BAD = range(5)
FIELDS = ("play", "queued", "complete", "ready", "span", "head", "inserted", "late", "ahead", "duplicate", "bad",
          "played_both", "played_md1", "played_md2", "played_none", "margin_min")
BOTH, MD1, MD2, NONE = range(4)


def queue_fields(q, play, depth):
    """(queued, complete, ready, span, head) of one stream: q = {seq: [lenA, lenB]}, every key inside [play, play + depth)"""
    filled = sorted(s for s, (la, lb) in q.items() if la or lb)
    assert all(play <= s < play + depth for s in filled)
    ready = 0
    while ready < depth and (play + ready) in q and any(q[play + ready]):
        ready += 1
    la, lb = q.get(play, (0, 0))
    return (len(filled), sum(1 for s in filled if q[s][0] and q[s][1]), ready, (filled[-1] - play + 1) if filled else 0,
            (1 if la else 0) | (2 if lb else 0))


def selected(ready, span, m, max_span):
    return ready >= m or m <= 0 or (max_span > 0 and span >= max_span)


def lens_words(queues, plays, depth):
    """the ring's length words [N][depth] for these queues: entry seq mod depth = lenA | lenB << 16"""
    w = np.zeros((len(queues), depth), np.uint32)
    for s, q in enumerate(queues):
        for seq, (la, lb) in q.items():
            assert plays[s] <= seq < plays[s] + depth
            w[s, seq % depth] = la | (lb << 16)
    return w


class RingModel:
    def __init__(self, n_streams, depth, slot, first_seq=0):
        self.N, self.D, self.slot = n_streams, depth, slot
        self.tracking = False
        self.cnt = None
        self.create(first_seq)

    def create(self, first_seq=0):
        self.play = [first_seq] * self.N
        self.q = [dict() for _ in range(self.N)]            # seq -> [lenA, lenB]
        self.src = [dict() for _ in range(self.N)]          # seq -> [arrival of A, arrival of B] (what was filed: offset, len)
        self.stats = [0] * 5
        if self.cnt is not None:
            self._zero(range(self.N))

    def _zero(self, streams):
        for s in streams:
            self.cnt[s] = [0] * 9
            self.margin[s] = self.D

    def track(self, on):
        if on:
            self.cnt = [[0] * 9 for _ in range(self.N)] if self.cnt is None else self.cnt
            self.margin = [self.D] * self.N
            self._zero(range(self.N))
        self.tracking = bool(on)

    def reset_streams(self, streams, first_seq):
        for s, f in zip(streams, first_seq):
            self.q[s], self.src[s], self.play[s] = dict(), dict(), f
        if self.cnt is not None:
            self._zero(streams)

    def insert(self, arrivals, payload_bytes, use_md_index, true_desc):
        """arrivals: rows (stream, seq, desc, offset, len); use_md_index: one flag per stream; true_desc: offset -> the description a
        payload really is (what the library reads off it when desc = -1).  Returns the verdicts."""
        out = []
        for s, seq, d, off, ln in arrivals:
            v = INSERTED
            if not (0 <= s < self.N) or d not in (-1, 0, 1) or ln <= 0 or ln > self.slot or ln > 0x7FFF or off < 0 or off + ln > payload_bytes or seq < 0:
                v = BAD
            elif seq < self.play[s]:
                v = LATE
            elif seq >= self.play[s] + self.D:
                v = AHEAD
            else:
                if d < 0:
                    d = true_desc[off] if use_md_index[s] else None
                if d is None:
                    v = BAD
                else:
                    e = self.q[s].setdefault(seq, [0, 0])
                    if e[d]:
                        v = DUP
                    else:
                        e[d] = ln
                        self.src[s].setdefault(seq, [None, None])[d] = (off, ln)
            self.stats[v] += 1
            if self.tracking and 0 <= s < self.N:
                self.cnt[s][v] += 1
                if v == INSERTED:
                    self.margin[s] = min(self.margin[s], seq - self.play[s])
            out.append(v)
        return out

    def play_out(self, streams, n_packets=1):
        """plays the next n_packets of the listed streams -> per stream a list of (seq, [arrival A, arrival B]) of what was queued"""
        out = []
        for s in streams:
            row = []
            for _ in range(n_packets):
                p = self.play[s]
                la, lb = self.q[s].pop(p, (0, 0))
                row.append((p, self.src[s].pop(p, [None, None])))
                if self.tracking:
                    self.cnt[s][5 + (BOTH if la and lb else MD1 if la else MD2 if lb else NONE)] += 1
                self.play[s] = p + 1
            out.append(row)
        return out

    def report(self, streams=None, min_ready=0, max_span=0, clear_margin=False):
        """-> (reports int64 [n, 16], play_list, play_rows): the list and the rows have `selected` entries"""
        streams = list(range(self.N)) if streams is None else list(streams)
        rep = np.zeros((len(streams), 16), np.int64)
        lst, rows = [], []
        for i, s in enumerate(streams):
            qd, cp, ready, span, head = queue_fields(self.q[s], self.play[s], self.D)
            cnt = self.cnt[s] if self.cnt is not None else [0] * 9
            rep[i] = [self.play[s], qd, cp, ready, span, head] + list(cnt) + [self.margin[s] if self.cnt is not None else self.D]
            m = min_ready if isinstance(min_ready, int) else int(min_ready[i])
            if selected(ready, span, m, max_span):
                lst.append(s); rows.append(i)
            if clear_margin and self.cnt is not None:
                self.margin[s] = self.D
        return rep, lst, rows

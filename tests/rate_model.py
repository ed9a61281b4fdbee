"""The rule of solo_rate (include/solo_mi355x.h) in plain Python integers: the controller's step for one row, the send mask, the meaning
of a value of solo_batch_update_rates, the parameter check -- and the constructed feedback sequences the tests run through it.  This
file is the normative text: the host build of solo_amd/csrc/solo_rate.h (tests/test_rate_model.py) and the kernels
(tests/test_gpu_rate.py) must equal it word for word.

A state record is 16 words: flags (1 started, 2 has used a report, 4 thin), target_bps, last_ehs (uint32), min_rtt, idle, over, under,
reports used and targets changed (uint32, since the reset), the last fraction_lost and rtt used, five words nobody writes."""
import numpy as np

WORDS, STATE_BYTES = 16, 64
I32_MAX = 2 ** 31 - 1
INIT = (0, 0, 0, I32_MAX) + (0,) * 12
LIVE = 11                                                   # the words a step may write
STARTED, HAS_REPORT, THIN = 1, 2, 4
BYE = 1 << 30
PARAMS = ("min_bps", "max_bps", "start_bps", "quantum_bps", "lo_q8", "hi_q8", "inc_q8", "rtt_guard", "stale_calls", "thin_after", "thin_release", "reserved")
# policy defaults of the binding, not measurements: the 2 % / 10 % thresholds and the 5 % step of the loss-based controller of the RMCAT
# "Google Congestion Control" draft
DEFAULTS = dict(quantum_bps=200, lo_q8=5, hi_q8=26, inc_q8=13, rtt_guard=0, stale_calls=250, thin_after=0, thin_release=3)
COUNT = ("rows", "started", "used", "repeated", "increased", "decreased", "held", "delayed", "stale", "bye", "thin_on", "thin_off", "thin_rows",
         "changed")
APPLY_COUNT = ("applied", "kept", "refused", "listed")


def params(min_bps, max_bps, start_bps, **kw):
    p = dict(DEFAULTS, min_bps=min_bps, max_bps=max_bps, start_bps=start_bps, reserved=0)
    for k, v in kw.items():
        assert k in PARAMS, k
        p[k] = v
    return p


def params_words(p):
    return np.array([p[k] for k in PARAMS], dtype=np.int32)


def params_ok(p):
    q = p["quantum_bps"]
    if q < 1 or p["min_bps"] < 1 or p["max_bps"] > 1000000 or not p["min_bps"] <= p["start_bps"] <= p["max_bps"]:
        return False
    if p["min_bps"] % q or p["max_bps"] % q or p["start_bps"] % q:
        return False
    if not 0 <= p["lo_q8"] <= p["hi_q8"] <= 255 or not 0 <= p["inc_q8"] <= 256:
        return False
    return min(p["rtt_guard"], p["stale_calls"], p["thin_after"], p["thin_release"]) >= 0 and p["reserved"] == 0


def _i32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >> 31 else v


def step(w, p, seen, fraction_lost, ext_high_seq, rtt, hits=None):
    """one row, one call: w the record's 16 words (changed in place) -> (d_target_bps, d_mode, the names of the counts the row adds to).
    hits: a set that collects which places of the rule the call went through"""
    hit = (lambda name: None) if hits is None else hits.add
    ev = set()
    changed = False
    if not w[0] & STARTED:                                  # 1
        w[:LIVE] = INIT[:LIVE]
        w[0], w[1] = STARTED, p["start_bps"]
        ev.add("started")
        changed = True
    if seen & BYE:                                          # 2
        w[:LIVE] = INIT[:LIVE]
        hit("bye_with_block" if seen & 0xFFFF else "bye_without_block")
        return 0, 0, ev | {"bye"}
    old = t = w[1]
    thin = bool(w[0] & THIN)
    ehs = ext_high_seq & 0xFFFFFFFF
    blocks = (seen & 0xFFFF) > 0
    used = blocks and (not w[0] & HAS_REPORT or _i32(ehs - w[2]) > 0)       # 3
    if blocks and not used:
        ev.add("repeated")
    if not used:                                            # 4
        before = w[4]
        w[4] = min(before + 1, I32_MAX)
        if p["stale_calls"] > 0 and before < p["stale_calls"] <= w[4]:
            hit("stale_lowers" if t > p["start_bps"] else "stale_keeps")
            t = min(t, p["start_bps"])
            thin = False
            w[5] = w[6] = 0
            ev.add("stale")
    else:                                                   # 5
        ev.add("used")
        if w[0] & HAS_REPORT and ehs < w[2]:
            hit("ehs_wrapped")
        w[7] = (w[7] + 1) & 0xFFFFFFFF
        w[4] = 0
        w[0] |= HAS_REPORT
        w[2] = ehs
        q = min(max(fraction_lost, 0), 255)
        hit("p_%d" % q if q in (0, 255) else "p_between")
        w[9], w[10] = q, rtt
        if rtt > 0:
            w[3] = min(w[3], rtt)
        else:
            hit("rtt_minus_one" if rtt == -1 else ("rtt_zero" if rtt == 0 else "rtt_negative"))
        delayed = p["rtt_guard"] > 0 and rtt > 0 and rtt - w[3] > p["rtt_guard"]
        if q > p["hi_q8"]:
            w[5] = min(w[5] + 1, I32_MAX) if t <= p["min_bps"] else 0
            a, b = t - (t * q >> 9), t - p["quantum_bps"]
            hit("decrease_by_factor" if a < b else "decrease_by_quantum")
            t = min(a, b)
            ev.add("decreased")
        else:
            w[5] = 0
            if q < p["lo_q8"] and not delayed and not thin:
                s = t * p["inc_q8"] >> 8
                hit("increase_by_factor" if s > p["quantum_bps"] else "increase_by_quantum")
                t += max(s, p["quantum_bps"])
                ev.add("increased")
            else:
                ev.add("held")
                if q < p["lo_q8"] and not thin:
                    ev.add("delayed")
                    hit("hold_by_delay")
                elif q < p["lo_q8"]:
                    hit("increase_refused_while_thin")
                else:
                    hit("hold_by_loss")
        if thin:                                            # 6
            w[6] = min(w[6] + 1, I32_MAX) if q < p["lo_q8"] else 0
            if w[6] >= p["thin_release"]:
                thin = False
                w[5] = w[6] = 0
                ev.add("thin_off")
        elif p["thin_after"] > 0 and w[5] >= p["thin_after"]:
            thin = True
            w[6] = 0
            ev.add("thin_on")
    if t < p["min_bps"]:
        hit("clamp_min")
    if t > p["max_bps"]:
        hit("clamp_max")
    t = min(max(t, p["min_bps"]), p["max_bps"])
    t -= t % p["quantum_bps"]
    w[1] = t
    w[0] = (w[0] & ~THIN) | (THIN if thin else 0)
    if t != old:
        changed = True
    if changed:
        ev.add("changed")
        w[8] = (w[8] + 1) & 0xFFFFFFFF
    if thin:
        ev.add("thin_rows")
    return (t if changed else 0), int(thin), ev


class Rate:
    """n_rows records and the calls of the object"""

    def __init__(self, n_rows):
        self.n_rows = n_rows
        self.w = [list(INIT) for _ in range(n_rows)]
        self.hits = set()

    def reset(self, rows=None):
        for r in (range(self.n_rows) if rows is None else rows):
            self.w[r] = list(INIT)

    def update(self, feedback, p):
        """feedback: n_rows rows of solo_rtcp_feedback_t as 8 integers -> (d_target_bps, d_mode, the count as a dict)"""
        assert params_ok(p) and len(feedback) == self.n_rows
        count = dict.fromkeys(COUNT, 0)
        count["rows"] = self.n_rows
        target, mode = [], []
        for w, f in zip(self.w, feedback):
            seen, fl, _, ehs, _, _, _, rtt = (int(v) for v in f)
            t, m, ev = step(w, p, _i32(seen), _i32(fl), ehs, _i32(rtt), self.hits)
            target.append(t)
            mode.append(m)
            for k in ev:
                count[k] += 1
        return np.array(target, dtype=np.int32), np.array(mode, dtype=np.uint8), count

    def state(self, rows=None):
        """the records as int32 [n, 16]: what get_state returns, seen as words"""
        rows = range(self.n_rows) if rows is None else rows
        return np.array([[_i32(v) for v in self.w[r]] for r in rows], dtype=np.int32).reshape(-1, WORDS)

    def set_state(self, words, rows=None):
        rows = range(len(words)) if rows is None else rows
        for r, rec in zip(rows, words):
            self.w[r] = [int(v) for v in rec]
            for k in (2, 7, 8):
                self.w[r][k] &= 0xFFFFFFFF


def list_ok(rows, n_rows):
    """the rule of every device list"""
    return all(0 <= v < n_rows for v in rows) and all(a < b for a, b in zip(rows, rows[1:]))


def mask(mode, seq, send_in=3):
    return ((2 if seq & 1 else 1) if mode else 3) & send_in


def send_mask(mode, n_packets, streams=None, seq_base=None, first_seq=0, send_in=None, n=None):
    """-> uint8 [n, n_packets], or None where the list is refused (nothing is written)"""
    if streams is not None and not list_ok(list(streams), len(mode)):
        return None
    rows = list(range(len(mode) if n is None else n)) if streams is None else list(streams)
    out = np.zeros((len(rows), n_packets), dtype=np.uint8)
    for i, r in enumerate(rows):
        for k in range(n_packets):
            seq = (first_seq + (0 if seq_base is None else int(seq_base[i])) + k) & 0xFFFFFFFF
            out[i, k] = mask(int(mode[r]), seq, 3 if send_in is None else int(send_in[i][k]))
    return out


def apply_target(target_bps, joint=False, wb=False):
    """a value of solo_batch_update_rates -> ("kept" | "refused" | "applied", the SILK rate that setup_rate takes, or None)"""
    if target_bps <= 0:
        return "kept", None
    silk = target_bps - (800 if joint else 1600)
    if wb and silk < 14000:
        return "refused", None
    return "applied", min(max(silk, 5000), 100000)


# ---- the constructed feedback sequences ------------------------------------------------------------------------------------------------
# Row r of call c belongs to family r % N_FAMILIES; v = r // N_FAMILIES varies the numbers.  The parameters that go with them put every
# threshold within reach of 40 calls.
N_FAMILIES = 8
CALLS = 40
TEST_PARAMS = params(6000, 40000, 16000, quantum_bps=400, rtt_guard=3000, stale_calls=4, thin_after=2, thin_release=2)
REQUIRED_HITS = {"bye_with_block", "bye_without_block", "stale_lowers", "ehs_wrapped", "p_0", "p_255", "p_between", "rtt_minus_one", "rtt_zero",
                 "decrease_by_factor", "decrease_by_quantum", "increase_by_factor", "increase_by_quantum", "hold_by_delay", "hold_by_loss",
                 "increase_refused_while_thin", "clamp_min", "clamp_max"}


def _lcg(x):
    return (1664525 * x + 1013904223) & 0xFFFFFFFF


def family(k, v, c):
    """(seen, fraction_lost, ext_high_seq, rtt) of family k, variant v, call c"""
    ehs = 100 + 7 * v + 25 * c
    rtt = 1000 + v
    if k == 0:                                              # clean: start, increases, the clamp at max_bps; fraction_lost 0
        return 1, 0, ehs, rtt
    if k == 1:                                              # heavy loss to the floor, thinning on; then clean: refused increases, thinning off
        return 1, (255 if c < 8 else 0), ehs, rtt
    if k == 2:                                              # hold by loss, then a loss just above hi_q8: decreases that end smaller than a quantum
        return 1 + v % 2, (10 if c < 5 else 27), ehs, rtt
    if k == 3:                                              # hold by delay; rtt -1 and 0 say nothing; a new minimum
        r = rtt if c < 3 else (rtt + 5000 if c < 7 else (-1 if c == 7 else (0 if c == 8 else (900 if c < 20 else 900 + 3001))))
        return 1, 0, ehs, r
    if k == 4:                                              # escalate, the same block again twice, silence: stale exactly at stale_calls
        if c < 6 or c > 20:
            return 1, 0, ehs, rtt
        return (1, 0, 100 + 7 * v + 25 * 5, rtt) if c < 8 else (0, 0, 0, -1)
    if k == 5:                                              # ext_high_seq through 2^32; a block that goes back
        e = (0xFFFFFF00 + 40 * (10 if c == 12 else c) + v) & 0xFFFFFFFF
        return 1, (30 if c % 2 else 0), e, rtt
    if k == 6:                                              # BYE with and without a block, and the restart behind each
        seen = 1 | BYE if c == 7 else (BYE if c == 15 else (0 if c == 16 else 1))
        return seen, 3, ehs, rtt
    x = _lcg(_lcg(0x5EED + 977 * v) ^ (c * 2654435761 & 0xFFFFFFFF))       # k == 7: anything, out-of-range fields included
    y = _lcg(x)
    return (x >> 9) % 3, (x >> 16) % 300 - 20, (100 + 25 * c - ((y >> 5) % 3) * 30) & 0xFFFFFFFF, (-1, 0, 500, 1500, 9000)[(y >> 12) % 5]


def feedback(n_rows, c):
    """int32 [n_rows, 8]: the rows of solo_rtcp_feedback_t of call c; the words the controller does not read are filled with noise"""
    out = np.zeros((n_rows, 8), dtype=np.int64)
    for r in range(n_rows):
        seen, fl, ehs, rtt = family(r % N_FAMILIES, r // N_FAMILIES, c)
        z = _lcg(r * 131 + c)
        out[r] = (seen, fl, z & 0xFFFFFF, ehs, z >> 7, z >> 3, z >> 11, rtt)
    return (out & 0xFFFFFFFF).astype(np.uint32).view(np.int32)

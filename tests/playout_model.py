"""Independent model of the play-out delay control (solo_playout_*), written from the rule as the interface states it and not from the
kernels: a row is a Python object, its observations are a plain list (no ring, no slots, no sorted insert -- the quantile is sorted()),
the lists are built by appending.  record() lays a row out as the 128-byte state record the interface documents, for the comparisons byte
for byte.  Used by tests/test_playout_model.py (against the host build of solo_playout.h) and tests/test_gpu_playout.py (against the GPU)."""
import numpy as np

IDLE, NORMAL, HELD, STRETCH, ACCEL, ACCEL_FORCED = range(6)                               # actions
OUTCOMES = ("idle", "normal", "held", "stretch", "stretch_gated", "accel", "accel_gated", "accel_forced")
O_IDLE, O_NORMAL, O_HELD, O_STRETCH, O_STRETCH_GATED, O_ACCEL, O_ACCEL_GATED, O_ACCEL_FORCED = range(8)
PARAMS = ("start_ready", "max_span", "window", "tolerate", "lo", "hi", "cooldown", "cost_gate")
DEFAULTS = dict(start_ready=2, max_span=0, window=16, tolerate=1, lo=1, hi=3, cooldown=8, cost_gate=0)
RING, NONE16, CUM_MAX, SLACK_MAX = 32, -32768, 16000, 1000
# columns of a solo_recv_report_t that the rule reads
READY, SPAN, LATE, MARGIN = 3, 4, 7, 15


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    assert set(p) == set(PARAMS)
    return p


def params_ok(p):
    return (p["start_ready"] >= 1 and p["max_span"] >= 0 and 1 <= p["window"] <= 32 and 0 <= p["tolerate"] <= 3 and 0 <= p["lo"] <= p["hi"] <= 64 and
            0 <= p["cooldown"] <= 1000)


class Row:
    def __init__(self, L):
        self.L = L
        self.run = self.held = self.cum = self.cool = self.age = self.late_prev = 0
        self.obs = None                                    # every observation since the start, oldest first; None = none
        self.raw = np.zeros(128, np.uint8)                 # the record as long as the row has never started (whatever it was reset to)
        self.held_pcm = np.zeros(L, np.int16)
        # what the tests ask about the run
        self.rule = None
        self.q_undefined = self.q_by_tolerate = False

    def record(self):
        """the 128 bytes of the interface"""
        if self.obs is None:
            return self.raw.copy()
        w = np.zeros(32, np.int32)
        w[:5] = [self.run, self.held, self.cum, self.cool, self.age]
        w[5] = np.array([self.late_prev], np.uint32).view(np.int32)[0]
        w[6] = len(self.obs) % RING
        ring = np.full(RING, NONE16, np.int16)
        for t in range(max(0, len(self.obs) - RING), len(self.obs)):
            if self.obs[t] is not None:
                ring[t % RING] = self.obs[t]
        w[8:24] = ring.view(np.int32)
        return w.view(np.uint8).copy()

    def ring_values(self):
        """the last 32 observations, oldest first (None = none)"""
        return list(self.obs[-RING:]) if self.obs else []


def decide(row, p, ready, span, late, margin_min, depth):
    """one tick of one row: the observation and the decision -> action; row.rule = the number of the rule that decided (1 .. 7)"""
    row.q_undefined = row.q_by_tolerate = False
    over = p["max_span"] > 0 and span >= p["max_span"]
    if not row.run:
        row.rule = 1
        if ready >= p["start_ready"] or over:
            row.run, row.held, row.cum, row.cool, row.age, row.late_prev, row.obs = 1, 0, 0, 0, 0, late, []
            return NORMAL
        return IDLE
    dl = (late - row.late_prev) % 2 ** 32
    row.late_prev = late
    if dl > 0:
        s = -1
    elif margin_min < depth:
        s = min(max(margin_min + row.held, -1), SLACK_MAX)
    else:
        s = None
    row.obs.append(None if s is None else s - row.cum)
    row.age = min(row.age + 1, p["window"])
    vals = sorted(v for v in row.obs[-row.age:] if v is not None)
    e = None
    if len(vals) > p["tolerate"]:
        e = vals[p["tolerate"]] + row.cum
        row.q_by_tolerate = vals[p["tolerate"]] != vals[0]
    else:
        row.q_undefined = True
    if row.held:
        row.rule, row.cool = 2, max(row.cool - 1, 0)
        return HELD
    if over:
        row.rule = 3
        return ACCEL_FORCED
    if row.cool > 0:
        row.rule, row.cool = 4, row.cool - 1
        return NORMAL
    if e is not None and e < p["lo"] and ready >= 1 and (p["max_span"] == 0 or span + 1 < p["max_span"]):
        row.rule = 5
        return STRETCH
    if row.age >= p["window"] and e is not None and e > p["hi"] and ready >= 2:
        row.rule = 6
        return ACCEL
    row.rule = 7
    return NORMAL


def list_ok(listed, n_rows):
    return all(0 <= s < n_rows for s in listed) and all(a < b for a, b in zip(listed, listed[1:]))


def plan(rows, listed, reports, p, depth):
    """rows: every Row of the object; listed: the rows of the call, in order; reports [n][16] -> dict(action, one, two, stretch_pos, count,
    where): where[i] = (position in one or two or None, position among the STRETCH rows or None).  A bad list: count n_one = -1 only."""
    if not list_ok(list(listed), len(rows)):
        return dict(count=dict(n_one=-1))
    action, one, two, spos, where = [], [], [], [], []
    for i, s in enumerate(listed):
        r = reports[i]
        a = decide(rows[s], p, int(r[READY]), int(r[SPAN]), int(r[LATE]) % 2 ** 32, int(r[MARGIN]), depth)
        action.append(a)
        k = j = None
        if a in (NORMAL, STRETCH):
            k = len(one)
            one.append(s)
            if a == STRETCH:
                j = len(spos)
                spos.append(k)
        elif a in (ACCEL, ACCEL_FORCED):
            k = len(two)
            two.append(s)
        where.append((k, j))
    return dict(action=action, one=one, two=two, stretch_pos=spos, where=where,
                count=dict(n_one=len(one), n_two=len(two), n_stretch=len(spos), listed=len(listed)))


def render(rows, listed, pl, p, pcm_one=None, st_one=None, pcm_two=None, st_two=None, ts_s=None, cost_s=None, ts_a=None, cost_a=None):
    """the execution of a plan: pcm_one [n_one][L], pcm_two [n_two][2][L], ts_s [n_stretch][2][L], cost_s [n_stretch][2M], ts_a [n_two][L],
    cost_a [n_two][M] -> (heard [n][L], outcome [n], status [n], count dict); held packets and held / cum / cool of the rows move"""
    n = len(listed)
    L = rows[0].L
    heard, outcome, status = np.zeros((n, L), np.int16), np.zeros(n, np.int32), np.zeros(n, np.int32)
    gate = p["cost_gate"]
    for i, s in enumerate(listed):
        row, a, (k, j) = rows[s], pl["action"][i], pl["where"][i]
        if a == IDLE:
            outcome[i] = O_IDLE
        elif a == NORMAL:
            heard[i], status[i], outcome[i] = pcm_one[k], st_one[k], O_NORMAL
        elif a == HELD:
            heard[i], outcome[i], row.held = row.held_pcm, O_HELD, 0
        elif a == STRETCH:
            status[i] = st_one[k]
            if gate > 0 and int(np.max(cost_s[j])) > gate:
                heard[i], outcome[i] = pcm_one[k], O_STRETCH_GATED
            else:
                heard[i], outcome[i] = ts_s[j][0], O_STRETCH
                row.held_pcm = np.array(ts_s[j][1], np.int16)
                row.held, row.cum, row.cool = 1, min(row.cum + 1, CUM_MAX), p["cooldown"]
        else:
            status[i] = st_two[k]
            if a == ACCEL and gate > 0 and int(np.max(cost_a[k])) > gate:
                heard[i], outcome[i] = pcm_two[k][0], O_ACCEL_GATED
                row.held_pcm = np.array(pcm_two[k][1], np.int16)
                row.held = 1
            else:
                heard[i] = np.asarray(ts_a[k]).reshape(L)
                outcome[i] = O_ACCEL if a == ACCEL else O_ACCEL_FORCED
                row.cum, row.cool = max(row.cum - 1, -CUM_MAX), p["cooldown"]
    count = {name: int((outcome == o).sum()) for o, name in enumerate(OUTCOMES)}
    return heard, outcome, status, count


def records(rows, which=None):
    which = range(len(rows)) if which is None else which
    return np.stack([rows[s].record() for s in which])


def held_store(rows, which=None):
    which = range(len(rows)) if which is None else which
    return np.stack([rows[s].held_pcm for s in which])


# ---- generated reports: what a network can do to a stream, one family per row ------------------------------------------------------------
FAMILIES = ("steady", "late_per_window", "late_burst", "drift_up", "dtx", "overflow", "startup_gaps", "late_wrap")


class ReportScript:
    """reports [n_rows][16] tick by tick for rows of the eight families (row r: family r mod 8, varied by r).  The columns the rule
    does not read carry noise: they must not matter."""

    def __init__(self, n_rows, depth, window, max_span, seed=1, lates=True):
        self.n, self.D, self.W, self.max_span, self.lates = n_rows, depth, window, max_span, lates
        self.rng = np.random.RandomState(seed)
        self.late = np.zeros(n_rows, np.int64)
        for r in range(n_rows):
            if FAMILIES[r % 8] == "late_wrap":
                self.late[r] = 2 ** 32 - 1 - (r // 8) % 3
        self.t = 0

    def tick(self):
        t, D = self.t, self.D
        rep = self.rng.randint(0, 1000, size=(self.n, 16)).astype(np.int64)
        for r in range(self.n):
            fam, v = FAMILIES[r % 8], r // 8
            ready, span, margin, dlate = 2, 2, 2, 0
            if fam == "steady":
                ready = span = 2 + v % 3
                margin = 1 + v % 3
            elif fam == "late_per_window":
                lates = 1 + v % 2                            # one late a window is tolerated, two are not
                if t % self.W < lates:
                    dlate = 1
            elif fam == "late_burst":
                if 10 + v % 5 <= t < 14 + v % 5:
                    dlate, ready, span = 2, 1, 1
                margin = 1
            elif fam == "drift_up":
                margin = min(1 + t // (3 + v % 4), D - 1)
                ready = span = min(margin + 1, D)
            elif fam == "dtx":
                if t > 3 + v % 4:
                    ready = span = 0
                    margin = D
            elif fam == "overflow":
                if t % (9 + v % 3) >= 7:
                    span = self.max_span + (v % 2)
                    ready = 1 + v % 4
                if t < 4:
                    ready = 0
                    span = self.max_span if v % 2 else 0      # a row that starts BY overflow
            elif fam == "startup_gaps":
                if t < 5 + v % 7:
                    ready, span, margin = t % 2, 3, D
                else:
                    margin = 0 if (t + v) % 5 == 0 else 1
            elif fam == "late_wrap":
                if t % 6 == 2:
                    dlate = 1 + v % 2
                margin = 3
            self.late[r] = (self.late[r] + (dlate if self.lates else 0)) % 2 ** 32
            rep[r, READY], rep[r, SPAN], rep[r, LATE], rep[r, MARGIN] = ready, span, self.late[r], margin
        self.t += 1
        return rep


def fake_decodes(rng, pl, L, M, silent_costs=False):
    """random stand-ins for what the decoder and the time scaler would deliver for a plan (the CPU tests have no decoder): every buffer
    the render reads"""
    c = pl["count"]
    n1, n2, ns = c["n_one"], c["n_two"], c["n_stretch"]

    def pcm(*shape):
        return rng.randint(-32768, 32768, size=shape).astype(np.int16)

    def cost(*shape):                                         # every other row stays below 20000, the rest below 60000
        c = rng.randint(0, 60001, size=shape) // np.where(np.arange(shape[0]) % 2, 1, 3)[:, None]
        return (np.zeros(shape) if silent_costs else c).astype(np.int32)
    return dict(pcm_one=pcm(n1, L), st_one=rng.randint(-3, 1, size=n1).astype(np.int32), pcm_two=pcm(n2, 2, L),
                st_two=rng.randint(-3, 1, size=n2).astype(np.int32), ts_s=pcm(ns, 2, L), cost_s=cost(ns, 2 * M), ts_a=pcm(n2, 1, L), cost_a=cost(n2, M))

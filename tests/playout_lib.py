"""What tests/test_playout_model.py (host build) and tests/test_gpu_playout.py (GPU) share: the host build of solo_playout.h as a ctypes
library, a back end that keeps an object's memory in numpy arrays, and drive(): the tick-by-tick comparison of a back end with the
independent model of tests/playout_model.py -- every action, list, count, output sample and state byte after every tick."""
import ctypes as C

import numpy as np

import playout_model as PM
from host_build import host_lib

GUARD = 3                                                         # entries / rows behind the call's
FILL_A, FILL_L, FILL_N, FILL_H, FILL_O, FILL_S = -7, -77, 0x5A5A5A5A, 0x1234, -5, -99


class Params(C.Structure):
    _fields_ = [(n, C.c_int32) for n in PM.PARAMS]


def c_params(p):
    return Params(*[int(p[k]) for k in PM.PARAMS])


def build_host():
    lib = host_lib("playout")
    P, V, I = C.POINTER(Params), C.c_void_p, C.c_int
    lib.emu_po_params_ok.argtypes = [P]
    lib.emu_po_list_ok.argtypes = [V, I, I]
    lib.emu_po_tick_call_ok.argtypes = [I] * 8 + [V, I, P, V, V, V, V]
    lib.emu_po_plan.argtypes = [V, I, V, V, V, V, I, I, P, V, V, V, V, V]
    lib.emu_po_gather.argtypes = [I, V, I, V, I, I, V]
    lib.emu_po_render.argtypes = [V, V, I, I, V, V, V, I, P, I, V, I, I, I] + [V] * 12
    return lib


def aligned(shape, dtype, fill=0):
    """an array whose first byte is 16-byte aligned (the interface's rule for PCM, reports and counts)"""
    nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
    raw = np.zeros(nbytes + 16, np.uint8)
    off = (-raw.ctypes.data) % 16
    a = raw[off:off + nbytes].view(dtype).reshape(shape)
    a[...] = fill
    return a


def reports_i32(rep):
    """model reports (int64, late as an unsigned number) -> the int32 words of solo_recv_report_t, 16-byte aligned"""
    a = aligned(rep.shape, np.int32)
    a[...] = (np.asarray(rep, np.int64) % 2 ** 32).astype(np.uint32).view(np.int32)
    return a


def ptr(a):
    return None if a is None else a.ctypes.data


class HostBackend:
    """an object in numpy memory, driven through the host build"""

    def __init__(self, lib, n_rows, L):
        self.lib, self.n_rows, self.L = lib, n_rows, L
        self.state = np.zeros((n_rows, 32), np.int32)
        self.held = aligned((n_rows, L), np.int16)
        self.slot = np.full(n_rows, -1, np.int32)
        self.sslot = np.full(n_rows, -1, np.int32)

    def plan(self, rep, listed, p, depth):
        n = self.n_rows if listed is None else len(listed)
        rows = None if listed is None else np.asarray(listed, np.int32)
        out = dict(action=np.full(n + GUARD, FILL_A, np.int32), one=np.full(n + GUARD, FILL_L, np.int32), two=np.full(n + GUARD, FILL_L, np.int32),
                   stretch_pos=np.full(n + GUARD, FILL_L, np.int32), count=aligned((4,), np.int32, FILL_N))
        r = reports_i32(rep)
        out["ret"] = self.lib.emu_po_plan(ptr(self.state), self.n_rows, ptr(self.slot), ptr(self.sslot), ptr(r), ptr(rows), n, depth, C.byref(c_params(p)),
                                          ptr(out["action"]), ptr(out["one"]), ptr(out["two"]), ptr(out["stretch_pos"]), ptr(out["count"]))
        return out

    def render(self, listed, p, block, action, dec):
        n, L = self.n_rows if listed is None else len(listed), self.L
        rows = None if listed is None else np.asarray(listed, np.int32)
        d = {k: (None if len(v) == 0 else _al(v)) for k, v in dec.items()}
        out = dict(heard=aligned((n + GUARD, L), np.int16, FILL_H), outcome=np.full(n + GUARD, FILL_O, np.int32), status=np.full(n + GUARD, FILL_S, np.int32),
                   count=aligned((8,), np.int32, FILL_N))
        act = np.ascontiguousarray(action, np.int32)
        out["ret"] = self.lib.emu_po_render(ptr(self.state), ptr(self.held), self.n_rows, L, ptr(self.slot), ptr(self.sslot), ptr(rows), n, C.byref(c_params(p)),
                                            block, ptr(act), len(dec["pcm_one"]), len(dec["pcm_two"]), len(dec["ts_s"]), ptr(d["pcm_one"]), ptr(d["st_one"]),
                                            ptr(d["pcm_two"]), ptr(d["st_two"]), ptr(d["ts_s"]), ptr(d["cost_s"]), ptr(d["ts_a"]), ptr(d["cost_a"]),
                                            ptr(out["heard"]), ptr(out["outcome"]), ptr(out["status"]), ptr(out["count"]))
        return out

    def get(self):
        return self.state.view(np.uint8).reshape(self.n_rows, 128).copy(), self.held.copy()

    def set(self, records, held):
        self.state[...] = np.ascontiguousarray(records, np.uint8).view(np.int32).reshape(self.n_rows, 32)
        self.held[...] = held


def _al(v):
    a = aligned(v.shape, v.dtype)
    a[...] = v
    return a


def check_plan(got, pl, n):
    """a back end's plan outputs against the model's, the entries beyond the counts and the guard entries still at their fill"""
    c = pl["count"]
    assert got["ret"] == 0
    assert dict(zip(("n_one", "n_two", "n_stretch", "listed"), got["count"].tolist())) == c
    assert got["action"][:n].tolist() == pl["action"] and (got["action"][n:] == FILL_A).all()
    for key, k in (("one", c["n_one"]), ("two", c["n_two"]), ("stretch_pos", c["n_stretch"])):
        assert got[key][:k].tolist() == pl[key], key
        assert (got[key][k:] == FILL_L).all(), key
    assert all(a < b for a, b in zip(pl["one"], pl["one"][1:])) and all(a < b for a, b in zip(pl["two"], pl["two"][1:]))


def check_render(got, want, n):
    heard, outcome, status, count = want
    assert got["ret"] == 0
    assert np.array_equal(got["outcome"][:n], outcome) and np.array_equal(got["status"][:n], status)
    bad = np.flatnonzero((got["heard"][:n] != heard).any(axis=1))
    assert len(bad) == 0, (bad[:8].tolist(), outcome[bad[:8]].tolist())
    assert dict(zip(PM.OUTCOMES, got["count"].tolist())) == count
    assert (got["heard"][n:] == FILL_H).all() and (got["outcome"][n:] == FILL_O).all() and (got["status"][n:] == FILL_S).all()   # the guard rows


class Seen:
    """what a run contained"""

    def __init__(self):
        self.actions, self.rules, self.outcomes = set(), set(), set()
        self.q_undefined = self.q_by_tolerate = False
        self.log = []                                        # per tick: (cool of the listed rows before the tick, the back end's actions, outcomes)

    def note(self, rows, listed, pl, outcome):
        self.actions |= set(pl["action"])
        self.outcomes |= set(int(o) for o in outcome)
        for s in listed:
            self.rules.add(rows[s].rule)
            self.q_undefined |= rows[s].q_undefined
            self.q_by_tolerate |= rows[s].q_by_tolerate


def drive(be, rows, script, listed, p, depth, block, ticks, seed, seen=None, silent_costs=False):
    """`ticks` ticks of plan + render on the back end `be` and on the model rows, compared after every stage; script.tick() gives the
    reports of ALL rows, the listed ones are handed on.  The decode and time-scaling outputs are random stand-ins."""
    rng = np.random.RandomState(seed)
    L, M = be.L, be.L // block
    ls = list(range(be.n_rows)) if listed is None else list(listed)
    n = len(ls)
    for _ in range(ticks):
        cool_before = be.get()[0].view(np.int32)[ls, 3].copy()
        rep = script.tick()[ls]
        pl = PM.plan(rows, ls, rep, p, depth)
        got = be.plan(rep, listed, p, depth)
        check_plan(got, pl, n)
        dec = PM.fake_decodes(rng, pl, L, M, silent_costs)
        want = PM.render(rows, ls, pl, p, **dec)
        out = be.render(listed, p, block, got["action"][:n], dec)
        check_render(out, want, n)
        state, held = be.get()
        assert np.array_equal(state, PM.records(rows)), np.flatnonzero((state != PM.records(rows)).any(axis=1))[:8]
        assert np.array_equal(held, PM.held_store(rows))
        if seen is not None:
            seen.note(rows, ls, pl, want[1])
            seen.log.append((cool_before, got["action"][:n].copy(), out["outcome"][:n].copy(), out["heard"][:n].copy(), dec, pl["where"]))


# ---- the render alone: crafted states, one plan tick, the render with a known largest cost ----------------------------------------------
CMAX = 40000
KINDS = ("idle", "normal", "held", "stretch", "accel", "forced")


def crafted_rows(Lr, n, p, rng):
    """model rows in states from which one plan tick gives a known action: row i is of kind i mod 6 -> (rows, reports)"""
    rows, rep = [PM.Row(Lr) for _ in range(n)], np.zeros((n, 16), np.int64)
    W = p["window"]
    for i, row in enumerate(rows):
        kind = KINDS[i % 6]
        ready, span, margin = 3, 3, 2
        if kind == "idle":
            ready = span = 0
        else:
            row.run, row.obs, row.age, row.cum, row.late_prev = 1, [2 - (i % 3)] * (W + i % 5), W, i % 3, 17
            if kind == "held":
                row.held, row.cool = 1, i % 2
                row.held_pcm = rng.randint(-32768, 32768, size=Lr).astype(np.int16)
            elif kind == "stretch":
                row.obs, margin = [-row.cum] * W, row.cum
            elif kind == "accel":
                row.obs, margin = [6 - row.cum] * W, 6
            elif kind == "forced":
                span, row.cool = p["max_span"], 2
        rep[i, PM.READY], rep[i, PM.SPAN], rep[i, PM.LATE], rep[i, PM.MARGIN] = ready, span, 17, margin
    return rows, rep


def render_case(make_backend, Lr, block, gate):
    """one plan tick from crafted states, then the render with every row's largest cost at CMAX; -> outcomes"""
    n, rng = 20, np.random.RandomState(Lr + max(gate, 0))
    p = PM.params(start_ready=2, max_span=6, window=8, tolerate=1, lo=1, hi=3, cooldown=5, cost_gate=gate)
    rows, rep = crafted_rows(Lr, n, p, rng)
    be = make_backend(n, Lr)
    be.set(PM.records(rows), PM.held_store(rows))
    pl = PM.plan(rows, list(range(n)), rep, p, 8)
    assert [KINDS[i % 6] for i in range(n)] == [("idle", "normal", "held", "stretch", "accel", "forced")[a] for a in pl["action"]]
    got = be.plan(rep, None, p, 8)
    check_plan(got, pl, n)
    dec = PM.fake_decodes(rng, pl, Lr, Lr // block)
    for key in ("cost_s", "cost_a"):
        dec[key] = np.minimum(dec[key], CMAX - 1)
        dec[key][np.arange(len(dec[key])), rng.randint(0, dec[key].shape[1], size=len(dec[key]))] = CMAX
    before = PM.records(rows).view(np.int32).copy()
    want = PM.render(rows, list(range(n)), pl, p, **dec)
    check_render(be.render(None, p, block, got["action"][:n], dec), want, n)
    state, held = be.get()
    assert np.array_equal(state, PM.records(rows)) and np.array_equal(held, PM.held_store(rows))
    # held / cum / cool after it, from the interface's table and not from the model
    after, out = state.view(np.int32), want[1]
    for i in range(n):
        b, a = before[i], after[i]
        exp = {PM.O_IDLE: (b[1], b[2], b[3]), PM.O_NORMAL: (b[1], b[2], b[3]), PM.O_HELD: (0, b[2], b[3]), PM.O_STRETCH: (1, b[2] + 1, 5),
               PM.O_STRETCH_GATED: (b[1], b[2], b[3]), PM.O_ACCEL: (b[1], b[2] - 1, 5), PM.O_ACCEL_GATED: (1, b[2], b[3]), PM.O_ACCEL_FORCED: (b[1], b[2] - 1, 5)}
        assert tuple(a[1:4]) == exp[int(out[i])], (i, out[i])
    return set(int(o) for o in out)


def simulate(be, arrivals, p, depth, block, seed=3, silent_costs=True):
    """a back end alone against a simulated network (the ring model of tests/recv_report_model.py): arrivals[t] = the (stream, seq,
    description) filed ahead of tick t.  Every tick files its arrivals, reports, plans, plays what the plan lists and renders random
    audio.  -> (per tick: actions, ring words [n][16] and pos [n] after the tick, outcomes; the ring model)"""
    from recv_report_model import RingModel
    n = be.n_rows
    ring = RingModel(n, depth, 256)
    ring.track(True)
    rng = np.random.RandomState(seed)
    log = []
    for arr in arrivals:
        ring.insert([(s, k, d, 0, 10) for s, k, d in arr], 100, [0] * n, {})
        rep = ring.report(None, clear_margin=True)[0]
        got = be.plan(rep, None, p, depth)
        assert got["ret"] == 0
        c = dict(zip(("n_one", "n_two", "n_stretch", "listed"), got["count"].tolist()))
        ring.play_out(got["one"][:c["n_one"]].tolist(), 1)
        ring.play_out(got["two"][:c["n_two"]].tolist(), 2)
        dec = PM.fake_decodes(rng, dict(count=c), be.L, be.L // block, silent_costs=silent_costs)
        out = be.render(None, p, block, got["action"][:n], dec)
        assert out["ret"] == 0
        w = be.get()[0].view(np.int32)
        log.append((got["action"][:n].copy(), w[:, 8:24].copy(), w[:, 6].copy(), out["outcome"][:n].copy()))
    return log, ring


# ---- the end-to-end schedule of tests/test_gpu_playout.py: what the network does to each of 12 streams -------------------------------------
E2E_NS, E2E_DEPTH, E2E_TICKS, E2E_PACKETS = 12, 8, 64, 80
E2E_PARAMS = PM.params(start_ready=2, max_span=6, window=8, tolerate=1, lo=1, hi=1, cooldown=4, cost_gate=0)
E2E_KINDS = ("on_time", "constant_delay", "delay_step", "description_loss", "outage_and_burst", "late_start")


def e2e_arrivals(ticks=E2E_TICKS, n_streams=E2E_NS, n_packets=E2E_PACKETS):
    """-> arrivals[t] = [(stream, seq, description)]: stream s is of kind s mod 6, the second stream of a kind is a variant of the first.
    Packet k is sent in tick k."""
    out = [[] for _ in range(ticks)]
    for s in range(n_streams):
        kind, v = E2E_KINDS[s % 6], s // 6
        for k in range(n_packets):
            at, descs = k, [0, 1]
            if kind == "constant_delay":
                at = k + 2 + v
            elif kind == "delay_step":                      # one tick later (v = 0) or earlier (v = 1) between packets 20 and 40
                at = k + (1 - 2 * v if 20 <= k < 40 else 0)
            elif kind == "description_loss":
                if k % 3 == 1:
                    descs.remove(1)
                if k % 5 == 2:
                    descs.remove(0)
                if v and k % 7 == 3:
                    descs = []
            elif kind == "outage_and_burst":                 # three packets held back, then six delivered ahead of their time
                o, b = (30, 44) if v == 0 else (24, 50)
                at = o + 3 if o <= k < o + 3 else (b if b <= k < b + 6 else k)
            elif kind == "late_start":
                at = k + 5 + 3 * v
            if at < ticks:
                out[at] += [(s, k, d) for d in descs]
    return out

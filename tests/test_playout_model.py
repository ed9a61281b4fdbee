"""Play-out delay control (solo_playout_*, solo_amd/csrc/solo_playout.h) without a GPU: plan, gather and render are compiled for the host by
this test (tests/playout_host.cpp through tests/playout_lib.py) and compared with the independent model of tests/playout_model.py -- every
action, list, count, output sample and state byte after every tick of 48 ticks over 300 rows of eight report families, with all rows and
with a list of 77 --, then the render alone at the three packet lengths with the cost gate swept across the largest cost, what the
interface promises whatever the model says, and the refusals clause by clause."""
import ctypes as C

import numpy as np
import pytest

import playout_lib as PL
import playout_model as PM

N, TICKS, DEPTH, L, BLOCK = 300, 48, 8, 320, 80
P_RUN = PM.params(start_ready=2, max_span=7, window=8, tolerate=1, lo=1, hi=3, cooldown=3, cost_gate=30000)
LISTED = sorted(np.random.RandomState(77).choice(N, 77, replace=False).tolist())


@pytest.fixture(scope="module")
def host():
    return PL.build_host()


@pytest.fixture(scope="module")
def full_run(host):
    """the 300-row / 48-tick run with all rows: done once, asked about by several tests"""
    be, rows, seen = PL.HostBackend(host, N, L), [PM.Row(L) for _ in range(N)], PL.Seen()
    PL.drive(be, rows, PM.ReportScript(N, DEPTH, P_RUN["window"], P_RUN["max_span"]), None, P_RUN, DEPTH, BLOCK, TICKS, seed=5, seen=seen)
    return seen


def test_sizes_and_params(host):
    assert host.emu_po_params_size() == 32 and host.emu_po_plan_count_size() == 16 and host.emu_po_render_count_size() == 32
    assert host.emu_po_count_size() == 48 and host.emu_po_state_bytes() == 128
    assert [host.emu_po_blob_row_bytes(l) for l in (320, 640, 1280)] == [128 + 640, 128 + 1280, 128 + 2560]
    assert host.emu_po_params_ok(C.byref(PL.c_params(PM.params()))) == 1 and host.emu_po_params_ok(None) == 0
    for k, bad in (("start_ready", (0, -1)), ("max_span", (-1,)), ("window", (0, 33)), ("tolerate", (-1, 4)), ("lo", (-1, 4)), ("hi", (0, 65)),
                   ("cooldown", (-1, 1001))):
        for v in bad:
            p = PM.params(**{k: v})
            assert not PM.params_ok(p) and host.emu_po_params_ok(C.byref(PL.c_params(p))) == 0, (k, v)
    for p in (PM.params(lo=0, hi=0), PM.params(lo=64, hi=64), PM.params(window=1, tolerate=3), PM.params(window=32, cooldown=1000, cost_gate=-5),
              PM.params(cooldown=0, max_span=2 ** 31 - 1, start_ready=2 ** 31 - 1)):
        assert PM.params_ok(p) and host.emu_po_params_ok(C.byref(PL.c_params(p))) == 1
    ok = np.array([4, 0, 299], np.int32)
    assert host.emu_po_list_ok(ok.ctypes.data, 3, 300) == 1
    for bad, n in (([4, 4], 2), ([300], 1), ([-1], 1), ([0], 0)):
        a = np.array(bad, np.int32)
        assert host.emu_po_list_ok(a.ctypes.data, n, 300) == 0
    assert host.emu_po_list_ok(None, 1, 300) == 0
    assert host.emu_po_geometry_ok(1, 320) == 1 and host.emu_po_geometry_ok(0, 320) == 0 and host.emu_po_geometry_ok(1, 0) == 0
    assert host.emu_po_geometry_ok(1, 324) == 0 and host.emu_po_geometry_ok(1, 1920) == 1 and host.emu_po_geometry_ok(1, 1928) == 0


def test_plan_all_rows_against_the_model(full_run):
    """300 rows cross the 256-row tile and leave a partial wavefront; drive() has compared everything after every tick.  On the model
    alone: the run held every action, every rule and both corners of the quantile"""
    seen = full_run
    assert seen.actions == set(range(6)), seen.actions
    assert seen.rules == set(range(1, 8)), seen.rules
    assert seen.q_undefined and seen.q_by_tolerate
    assert seen.outcomes == set(range(8)), seen.outcomes


def test_plan_listed_rows_against_the_model(host):
    """all rows for 20 ticks, then a list of 77 for 28: the records and held packets of the 223 others stay bit for bit (drive() compares
    all 300 after every tick, and the model does not touch an unlisted row)"""
    be, rows = PL.HostBackend(host, N, L), [PM.Row(L) for _ in range(N)]
    script = PM.ReportScript(N, DEPTH, P_RUN["window"], P_RUN["max_span"], seed=2)
    PL.drive(be, rows, script, None, P_RUN, DEPTH, BLOCK, 20, seed=6)
    state0, held0 = be.get()
    assert len(LISTED) == 77 and (state0.view(np.int32)[:, 0] == 1).sum() > 200
    seen = PL.Seen()
    PL.drive(be, rows, script, LISTED, P_RUN, DEPTH, BLOCK, TICKS - 20, seed=7, seen=seen)
    state1, held1 = be.get()
    others = np.setdiff1d(np.arange(N), LISTED)
    assert np.array_equal(state0[others], state1[others]) and np.array_equal(held0[others], held1[others])
    assert not np.array_equal(state0[LISTED], state1[LISTED]) and {PM.STRETCH, PM.ACCEL, PM.HELD} <= seen.actions


def test_a_bad_list_writes_only_the_count(host):
    be = PL.HostBackend(host, N, L)
    rep = PM.ReportScript(N, DEPTH, 8, 7).tick()
    for bad in ([5, 5, 9], [9, 5, 12], [-1, 3, 4], [3, 4, N]):
        got = be.plan(rep[:3], bad, P_RUN, DEPTH)
        assert got["ret"] == 1 and got["count"].tolist() == [-1] + [PL.FILL_N] * 3
        assert all((got[k] == f).all() for k, f in (("action", PL.FILL_A), ("one", PL.FILL_L), ("two", PL.FILL_L), ("stretch_pos", PL.FILL_L)))
        assert not be.state.any() and (be.slot == -1).all()
        assert PM.plan([PM.Row(L) for _ in range(N)], bad, rep[:3], P_RUN, DEPTH)["count"] == dict(n_one=-1)
        dec = PM.fake_decodes(np.random.RandomState(1), dict(count=dict(n_one=0, n_two=0, n_stretch=0)), L, L // BLOCK)
        out = be.render(bad, P_RUN, BLOCK, np.zeros(3, np.int32), dec)
        assert out["ret"] == 1 and out["count"].tolist() == [-1] + [PL.FILL_N] * 7 and (out["heard"] == PL.FILL_H).all() and (out["outcome"] == PL.FILL_O).all()


# ---- the render alone ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Lr,block", ((320, 80), (640, 80), (1280, 160)))
def test_render_against_the_model_and_the_gate_sweep(host, Lr, block):
    """off and at / above the largest cost accept, below it gates (ACCEL_FORCED is never gated); together all eight outcomes"""
    mk = lambda n, l: PL.HostBackend(host, n, l)
    accepted = {PM.O_IDLE, PM.O_NORMAL, PM.O_HELD, PM.O_STRETCH, PM.O_ACCEL, PM.O_ACCEL_FORCED}
    gated = {PM.O_IDLE, PM.O_NORMAL, PM.O_HELD, PM.O_STRETCH_GATED, PM.O_ACCEL_GATED, PM.O_ACCEL_FORCED}
    assert PL.render_case(mk, Lr, block, 0) == accepted and PL.render_case(mk, Lr, block, -3) == accepted
    assert PL.render_case(mk, Lr, block, PL.CMAX - 1) == gated and PL.render_case(mk, Lr, block, 1) == gated
    assert PL.render_case(mk, Lr, block, PL.CMAX) == accepted and PL.render_case(mk, Lr, block, PL.CMAX + 1) == accepted
    assert accepted | gated == set(range(8))


def test_gather(host):
    rng = np.random.RandomState(4)
    pcm = PL.aligned((9, L), np.int16)
    pcm[...] = rng.randint(-32768, 32768, size=(9, L))
    spos = np.array([1, 4, 8], np.int32)
    out = PL.aligned((3 + PL.GUARD, L), np.int16, PL.FILL_H)
    assert host.emu_po_gather(N, pcm.ctypes.data, 9, spos.ctypes.data, 3, L, out.ctypes.data) == 0
    assert np.array_equal(out[:3], pcm[[1, 4, 8]]) and (out[3:] == PL.FILL_H).all()
    assert host.emu_po_gather(N, pcm.ctypes.data, 9, spos.ctypes.data, 0, L, out.ctypes.data) == -1
    assert host.emu_po_gather(N, pcm.ctypes.data, 2, spos.ctypes.data, 3, L, out.ctypes.data) == -1
    assert host.emu_po_gather(N, pcm.ctypes.data + 2, 9, spos.ctypes.data, 3, L, out.ctypes.data) == -1


# ---- what the interface promises, whatever the model says ------------------------------------------------------------------------------------
def test_held_follows_a_stretch_and_nothing_moves_while_cooling(full_run):
    log = full_run.log
    n_stretch = n_cooling = 0
    for t, (cool, action, outcome, _, _, _) in enumerate(log):
        moved = (action == PM.STRETCH) | (action == PM.ACCEL)
        assert not (moved & (cool > 0)).any()                               # never while cool > 0 ...
        n_cooling += int(((action == PM.ACCEL_FORCED) & (cool > 0)).sum())  # ... unless forced
        if t + 1 < len(log):
            nxt = log[t + 1][1]
            for o in (PM.O_STRETCH, PM.O_ACCEL_GATED):                      # something was put into the held store: it is played next
                assert (nxt[outcome == o] == PM.HELD).all()
            n_stretch += int((outcome == PM.O_STRETCH).sum())
    assert n_stretch >= 10 and n_cooling > 0


def test_wide_open_thresholds_play_every_packet_as_it_is(host):
    """lo = 0, hi = 64, max_span = 0: a running row is NORMAL forever and d_heard is the plain decode.  (Without late arrivals: a late one
    is slack -1, below any lo.)"""
    p = PM.params(start_ready=2, max_span=0, window=8, tolerate=0, lo=0, hi=64, cooldown=3, cost_gate=0)
    be, rows, seen = PL.HostBackend(host, N, L), [PM.Row(L) for _ in range(N)], PL.Seen()
    PL.drive(be, rows, PM.ReportScript(N, DEPTH, 8, 7, seed=9, lates=False), None, p, DEPTH, BLOCK, 24, seed=8, seen=seen)
    started = np.zeros(N, bool)
    for cool, action, outcome, heard, dec, where in seen.log:
        assert set(action.tolist()) <= {PM.IDLE, PM.NORMAL} and not (started & (action != PM.NORMAL)).any()
        started |= action == PM.NORMAL
        k = np.array([w[0] if w[0] is not None else -1 for w in where])
        assert np.array_equal(heard[action == PM.NORMAL], dec["pcm_one"][k[action == PM.NORMAL]]) and not heard[action == PM.IDLE].any()
    assert started.sum() > 250


def _schedule(n_packets=60):
    """arrival ticks of packet k: just in time for 20 ticks, then three ticks early (a burst, then one a tick again); never later"""
    return [k if k < 23 else max(k - 3, 20) for k in range(n_packets)]


def test_the_ring_does_not_move_when_play_out_does(host):
    """one arrival schedule under two parameter sets that differ only in cooldown: the actions differ, the stored observations do not
    (tick for tick, slot for slot).  No arrival is late in either run -- a late arrival is slack -1 whatever the delay, so it is the one
    thing that does depend on where play-out stands."""
    n, depth, ticks = 4, 16, 56
    arrivals = [[(s, k, 0) for s in range(n) for k, at in enumerate(_schedule()) if at == t] for t in range(ticks)]
    runs = []
    for cooldown in (0, 6):
        p = PM.params(start_ready=1, max_span=0, window=8, tolerate=0, lo=2, hi=3, cooldown=cooldown, cost_gate=0)
        log, ring = PL.simulate(PL.HostBackend(host, n, L), arrivals, p, depth, BLOCK)
        assert ring.stats[1] == 0 and ring.stats[2] == 0                    # nothing late, nothing ahead
        runs.append(log)
    a, b = runs
    assert any(not np.array_equal(x[0], y[0]) for x, y in zip(a, b))        # the actions differ ...
    for t, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x[1], y[1]) and np.array_equal(x[2], y[2]), t  # ... the rings are equal
    for log in runs:
        seen = set(int(o) for x in log for o in x[3])
        assert {PM.O_STRETCH, PM.O_HELD, PM.O_ACCEL, PM.O_NORMAL} <= seen


def test_the_end_to_end_schedule_reaches_every_outcome(host):
    """on the host build alone (no GPU, no audio): the schedule that tests/test_gpu_playout.py plays through the codec holds every outcome
    but the gated ones with the gate off, and both gated ones in a shorter run with a low gate"""
    def outcomes(ticks, gate):
        p = dict(PL.E2E_PARAMS, cost_gate=gate)
        log, ring = PL.simulate(PL.HostBackend(host, PL.E2E_NS, 640), PL.e2e_arrivals(ticks), p, PL.E2E_DEPTH, 80, silent_costs=False)
        assert max(ring.play) <= PL.E2E_PACKETS and ring.stats[1] > 0          # no packet is played that was never sent; some arrive late
        return set(int(o) for x in log for o in x[3])
    assert outcomes(PL.E2E_TICKS, 0) == set(range(8)) - {PM.O_STRETCH_GATED, PM.O_ACCEL_GATED}
    assert {PM.O_STRETCH_GATED, PM.O_ACCEL_GATED} <= outcomes(40, 1)


# ---- refusals: one assertion per clause of the header's "returns -1" sentences ------------------------------------------------------------
def test_plan_and_render_refusals(host):
    be = PL.HostBackend(host, 12, L)
    p, rep = PL.c_params(P_RUN), PL.reports_i32(np.zeros((12 + 1, 16), np.int64))
    rows = np.arange(12, dtype=np.int32)
    act, one, two, sp = (np.full(12, PL.FILL_A, np.int32) for _ in range(4))
    cnt = PL.aligned((8,), np.int32, PL.FILL_N)

    def plan(state=be.state.ctypes.data, reports=rep.ctypes.data, rws=None, n=12, depth=DEPTH, prm=C.byref(p), a=act.ctypes.data, o=one.ctypes.data,
             t=two.ctypes.data, s=sp.ctypes.data, c=cnt.ctypes.data):
        return host.emu_po_plan(state, 12, be.slot.ctypes.data, be.sslot.ctypes.data, reports, rws, n, depth, prm, a, o, t, s, c)

    assert plan(reports=None) == -1 and plan(a=None) == -1 and plan(o=None) == -1 and plan(t=None) == -1 and plan(s=None) == -1 and plan(c=None) == -1
    assert plan(prm=None) == -1 and plan(prm=C.byref(PL.c_params(PM.params(window=33)))) == -1
    assert plan(n=0) == -1 and plan(n=13) == -1 and plan(n=11) == -1 and plan(depth=0) == -1          # (n = 11 without a list)
    assert plan(reports=rep.ctypes.data + 4) == -1 and plan(c=cnt.ctypes.data + 4) == -1              # not 16-byte aligned
    assert all((x == PL.FILL_A).all() for x in (act, one, two, sp)) and (cnt == PL.FILL_N).all() and not be.state.any()
    assert plan(rws=rows.ctypes.data, n=11) == 0 and cnt[3] == 11

    pcm = PL.aligned((12, 2, L), np.int16)
    st, cost = np.zeros(12, np.int32), np.zeros((12, 8), np.int32)
    heard, outc, stat = PL.aligned((12, L), np.int16, PL.FILL_H), np.full(12, PL.FILL_O, np.int32), np.full(12, PL.FILL_S, np.int32)
    cnt[...] = PL.FILL_N
    state0 = be.state.copy()

    def render(rws=None, n=12, prm=C.byref(p), block=BLOCK, a=act.ctypes.data, n1=4, n2=3, ns=2, p1=pcm.ctypes.data, s1=st.ctypes.data, p2=pcm.ctypes.data,
               s2=st.ctypes.data, ts=pcm.ctypes.data, cs=cost.ctypes.data, ta=pcm.ctypes.data, ca=cost.ctypes.data, h=heard.ctypes.data, o=outc.ctypes.data,
               s=stat.ctypes.data, c=cnt.ctypes.data):
        return host.emu_po_render(be.state.ctypes.data, be.held.ctypes.data, 12, L, be.slot.ctypes.data, be.sslot.ctypes.data, rws, n, prm, block, a, n1, n2, ns,
                                  p1, s1, p2, s2, ts, cs, ta, ca, h, o, s, c)

    assert render(a=None) == -1 and render(h=None) == -1 and render(o=None) == -1 and render(s=None) == -1 and render(prm=None) == -1
    assert render(prm=C.byref(PL.c_params(PM.params(lo=5, hi=4)))) == -1
    assert render(n=0) == -1 and render(n=13) == -1 and render(n=11) == -1
    assert render(block=0) == -1 and render(block=70) == -1 and render(block=16) == -1                # 2 x 320 / 16 = 40 blocks > 32
    assert render(n1=-1) == -1 and render(n2=-1) == -1 and render(ns=-1) == -1 and render(ns=5) == -1 and render(n1=10, n2=3) == -1
    assert render(p1=None) == -1 and render(s1=None) == -1 and render(p2=None) == -1 and render(s2=None) == -1
    assert render(ts=None) == -1 and render(cs=None) == -1 and render(ta=None) == -1 and render(ca=None) == -1
    for k in ("p1", "p2", "ts", "ta", "h"):
        assert render(**{k: pcm.ctypes.data + 2}) == -1, k
    assert render(c=cnt.ctypes.data + 4) == -1
    assert (heard == PL.FILL_H).all() and (outc == PL.FILL_O).all() and (stat == PL.FILL_S).all() and (cnt == PL.FILL_N).all()
    assert np.array_equal(be.state, state0)
    assert render(n1=0, n2=0, ns=0, p1=None, s1=None, p2=None, s2=None, ts=None, cs=None, ta=None, ca=None, c=None) == 0   # empty lists, no count


def test_tick_refusals(host):
    p = PL.c_params(P_RUN)
    buf = PL.aligned((64,), np.int32)
    good = dict(n_rows=12, L=640, ring=1, tracking=1, h_streams=12, h_depth=8, h_L=640, h_fs=16000, rows=None, n=12, p=C.byref(p), heard=buf.ctypes.data,
                outcome=buf.ctypes.data, status=buf.ctypes.data, count=buf.ctypes.data)

    def ok(**kw):
        a = dict(good)
        a.update(kw)
        return host.emu_po_tick_call_ok(*[a[k] for k in ("n_rows", "L", "ring", "tracking", "h_streams", "h_depth", "h_L", "h_fs", "rows", "n", "p", "heard",
                                                          "outcome", "status", "count")])

    assert ok() == 1 and ok(rows=buf.ctypes.data, n=5) == 1 and ok(L=1280, h_L=1280, h_fs=32000) == 1
    assert ok(ring=0) == 0                                      # a handle without a ring
    assert ok(h_depth=1) == 0                                   # ... with a ring shallower than 2
    assert ok(tracking=0) == 0                                  # tracking off
    assert ok(h_streams=13) == 0 and ok(h_L=1280) == 0          # stream count or packet samples differ from the object's
    assert ok(h_fs=8000) == 0 and ok(L=1920, h_L=1920, h_fs=48000) == 0 and ok(L=648, h_L=648) == 0        # a packet the time scaler does not take
    assert ok(p=None) == 0 and ok(p=C.byref(PL.c_params(PM.params(tolerate=4)))) == 0
    assert ok(heard=None) == 0 and ok(outcome=None) == 0 and ok(status=None) == 0 and ok(count=None) == 0
    assert ok(n=0) == 0 and ok(n=13) == 0 and ok(n=5) == 0
    assert ok(heard=buf.ctypes.data + 4) == 0 and ok(count=buf.ctypes.data + 8) == 0

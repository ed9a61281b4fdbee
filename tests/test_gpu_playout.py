"""Play-out delay control on the GPU (solo_playout_* through solo_amd.Playout and through the raw C ABI, alternately): the 300-row / 48-tick
plan + render run and the render cases of tests/test_playout_model.py against the independent model of tests/playout_model.py, the state
round trip, and the tick end to end -- the reference encoder's packets under a scripted network, every d_heard sample, outcome, status and
count against the model of the rule driving the compiled reference decoder and the time-scaling model; the same schedule by hand on a twin
handle; the list refusal on the device; a side stream."""
import ctypes as C

import numpy as np
import pytest

import playout_lib as PL
import playout_model as PM
import refcodec as R
from recv_report_model import RingModel
from timescale_model import model_timescale

need_ref = pytest.mark.skipif(not R.have_ref("fix"), reason="oracle/_ref not present")
pytestmark = pytest.mark.gpu
N, TICKS, DEPTH, L, BLOCK = 300, 48, 8, 320, 80
P_RUN = PM.params(start_ready=2, max_span=7, window=8, tolerate=1, lo=1, hi=3, cooldown=3, cost_gate=30000)
LISTED = sorted(np.random.RandomState(77).choice(N, 77, replace=False).tolist())


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch


class GpuBackend:
    """a solo_amd.Playout behind the interface of playout_lib.HostBackend; every other call goes through the raw C ABI into pre-filled
    buffers with guard entries, the rest through the binding (whose fresh outputs are zero beyond what the call wrote)"""

    def __init__(self, torch, n_rows, Lr):
        import solo_amd
        self.t, self.n_rows, self.L, self.calls = torch, n_rows, Lr, 0
        self.po = solo_amd.Playout(n_rows, Lr)

    def _dev(self, a):
        return self.t.from_numpy(np.ascontiguousarray(a)).cuda()

    def _rows(self, listed):
        return None if listed is None else self._dev(np.asarray(listed, np.int32))

    def plan(self, rep, listed, p, depth):
        t, po = self.t, self.po
        n = self.n_rows if listed is None else len(listed)
        rows, d_rep = self._rows(listed), self._dev(PL.reports_i32(rep))
        self.calls += 1
        keys = ("action", "one", "two", "stretch_pos")
        fills = dict(action=PL.FILL_A, one=PL.FILL_L, two=PL.FILL_L, stretch_pos=PL.FILL_L)
        if self.calls % 2:
            d = {k: t.full((n + PL.GUARD,), fills[k], dtype=t.int32, device="cuda") for k in keys}
            cnt = t.full((4,), PL.FILL_N, dtype=t.int32, device="cuda")
            ret = po.lib.solo_playout_plan(po.h, d_rep.data_ptr(), None if rows is None else rows.data_ptr(), n, depth, C.byref(po.params(**p)),
                                           d["action"].data_ptr(), d["one"].data_ptr(), d["two"].data_ptr(), d["stretch_pos"].data_ptr(), cnt.data_ptr(),
                                           po._stream())
            out = {k: d[k].cpu().numpy() for k in keys}
            out["count"], out["ret"] = cnt.cpu().numpy(), ret
            return out
        got = po.plan(d_rep, depth, rows=rows, **p)
        c = po.count(got["count"])
        out = dict(ret=0, count=np.array([c["n_one"], c["n_two"], c["n_stretch"], c["listed"]], np.int32))
        for k, m in (("action", n), ("one", c["n_one"]), ("two", c["n_two"]), ("stretch_pos", c["n_stretch"])):
            x = got[k].cpu().numpy()
            assert not x[max(m, 0):].any()                          # (nothing written beyond the count)
            out[k] = np.concatenate([x[:max(m, 0)], np.full(n + PL.GUARD - max(m, 0), fills[k], np.int32)])
        return out

    def render(self, listed, p, block, action, dec):
        t, po, Lr = self.t, self.po, self.L
        n = self.n_rows if listed is None else len(listed)
        rows, act = self._rows(listed), self._dev(np.asarray(action, np.int32))
        d = {k: (None if len(v) == 0 else self._dev(v)) for k, v in dec.items()}
        self.calls += 1
        if self.calls % 2:
            heard = t.full((n + PL.GUARD, Lr), PL.FILL_H, dtype=t.int16, device="cuda")
            outc = t.full((n + PL.GUARD,), PL.FILL_O, dtype=t.int32, device="cuda")
            stat = t.full((n + PL.GUARD,), PL.FILL_S, dtype=t.int32, device="cuda")
            cnt = t.full((8,), PL.FILL_N, dtype=t.int32, device="cuda")
            ptr = lambda k: None if d[k] is None else d[k].data_ptr()
            ret = po.lib.solo_playout_render(po.h, None if rows is None else rows.data_ptr(), n, C.byref(po.params(**p)), block, act.data_ptr(),
                                             len(dec["pcm_one"]), len(dec["pcm_two"]), len(dec["ts_s"]), ptr("pcm_one"), ptr("st_one"), ptr("pcm_two"),
                                             ptr("st_two"), ptr("ts_s"), ptr("cost_s"), ptr("ts_a"), ptr("cost_a"), heard.data_ptr(), outc.data_ptr(),
                                             stat.data_ptr(), cnt.data_ptr(), po._stream())
            return dict(ret=ret, heard=heard.cpu().numpy(), outcome=outc.cpu().numpy(), status=stat.cpu().numpy(), count=cnt.cpu().numpy())
        heard, outc, stat, cnt = po.render(act, block, pcm_one=d["pcm_one"], status_one=d["st_one"], pcm_two=d["pcm_two"], status_two=d["st_two"],
                                           ts_stretch=d["ts_s"], cost_stretch=d["cost_s"], ts_accel=d["ts_a"], cost_accel=d["cost_a"], rows=rows, **p)
        pad = lambda x, f: np.concatenate([x.cpu().numpy(), np.full((PL.GUARD,) + tuple(x.shape[1:]), f, x.cpu().numpy().dtype)])
        return dict(ret=0, heard=pad(heard, PL.FILL_H), outcome=pad(outc, PL.FILL_O), status=pad(stat, PL.FILL_S), count=cnt.cpu().numpy())

    def get(self):
        blob = self.po.get_state().cpu().numpy()
        return blob[:, :128].copy(), blob[:, 128:].copy().view(np.int16)

    def set(self, records, held):
        blob = np.concatenate([np.ascontiguousarray(records, np.uint8), np.ascontiguousarray(held, np.int16).view(np.uint8)], axis=1)
        self.po.set_state(self._dev(blob))


def test_gpu_plan_and_render_against_the_model(torch_cuda):
    """the 300-row / 48-tick run: all rows, and (after 20 ticks of all) the list of 77"""
    be, rows, seen = GpuBackend(torch_cuda, N, L), [PM.Row(L) for _ in range(N)], PL.Seen()
    PL.drive(be, rows, PM.ReportScript(N, DEPTH, P_RUN["window"], P_RUN["max_span"]), None, P_RUN, DEPTH, BLOCK, TICKS, seed=5, seen=seen)
    assert seen.actions == set(range(6)) and seen.rules == set(range(1, 8)) and seen.q_undefined and seen.q_by_tolerate and seen.outcomes == set(range(8))
    be, rows = GpuBackend(torch_cuda, N, L), [PM.Row(L) for _ in range(N)]
    script = PM.ReportScript(N, DEPTH, P_RUN["window"], P_RUN["max_span"], seed=2)
    PL.drive(be, rows, script, None, P_RUN, DEPTH, BLOCK, 20, seed=6)
    state0, held0 = be.get()
    PL.drive(be, rows, script, LISTED, P_RUN, DEPTH, BLOCK, TICKS - 20, seed=7)
    state1, held1 = be.get()
    others = np.setdiff1d(np.arange(N), LISTED)
    assert np.array_equal(state0[others], state1[others]) and np.array_equal(held0[others], held1[others])
    assert not np.array_equal(state0[LISTED], state1[LISTED])


@pytest.mark.parametrize("Lr,block", ((320, 80), (640, 80), (1280, 160)))
def test_gpu_render_cases_and_the_gate_sweep(torch_cuda, Lr, block):
    mk = lambda n, l: GpuBackend(torch_cuda, n, l)
    accepted = {PM.O_IDLE, PM.O_NORMAL, PM.O_HELD, PM.O_STRETCH, PM.O_ACCEL, PM.O_ACCEL_FORCED}
    gated = {PM.O_IDLE, PM.O_NORMAL, PM.O_HELD, PM.O_STRETCH_GATED, PM.O_ACCEL_GATED, PM.O_ACCEL_FORCED}
    assert PL.render_case(mk, Lr, block, 0) == accepted
    assert PL.render_case(mk, Lr, block, PL.CMAX - 1) == gated
    assert PL.render_case(mk, Lr, block, PL.CMAX) == accepted and PL.render_case(mk, Lr, block, PL.CMAX + 1) == accepted


def test_gpu_gather(torch_cuda):
    torch = torch_cuda
    import solo_amd
    po = solo_amd.Playout(16, 640)
    pcm = torch.randint(-32768, 32768, (9, 640), dtype=torch.int16, device="cuda")
    out = po.gather(pcm, torch.tensor([1, 4, 8, 0], dtype=torch.int32, device="cuda"), 3)
    assert tuple(out.shape) == (3, 1, 640) and bool((out[:, 0] == pcm[[1, 4, 8]]).all())


def test_gpu_state_round_trip(torch_cuda):
    """get_state -> reset_rows -> set_state on 9 of 70 rows: the run continues bit for bit"""
    n = 70
    be, rows = GpuBackend(torch_cuda, n, L), [PM.Row(L) for _ in range(n)]
    script = PM.ReportScript(n, DEPTH, P_RUN["window"], P_RUN["max_span"], seed=4)
    PL.drive(be, rows, script, None, P_RUN, DEPTH, BLOCK, 14, seed=11)
    pick = [0, 3, 5, 9, 20, 33, 47, 68, 69]
    state0, held0 = be.get()
    assert (state0.view(np.int32)[pick, 0] == 1).sum() >= 7 and state0.view(np.int32)[pick, 1].any()      # running rows, a held packet among them
    blob = be.po.get_state(rows=pick)
    assert tuple(blob.shape) == (9, 128 + 2 * L) and np.array_equal(blob.cpu().numpy()[:, :128], state0[pick])
    be.po.reset_rows(pick[::-1])
    state, held = be.get()
    others = np.setdiff1d(np.arange(n), pick)
    assert not state[pick].any() and not held[pick].any() and np.array_equal(state[others], state0[others]) and np.array_equal(held[others], held0[others])
    be.po.set_state(blob, rows=pick)
    state, held = be.get()
    assert np.array_equal(state, state0) and np.array_equal(held, held0)
    PL.drive(be, rows, script, None, P_RUN, DEPTH, BLOCK, 14, seed=12)
    be.po.reset()
    state, held = be.get()
    assert not state.any() and not held.any()


# ---- the tick, end to end ------------------------------------------------------------------------------------------------------------------
N_SRC = 3


def _packets(n_packets):
    """N_SRC streams of the reference encoder's packets at 13.6 kbps (stream s of the run sends source s mod N_SRC) -> (recs[src][k] =
    (packet, n0, n1), parts {(src, k, d): (offset, len)}, payload pool)"""
    recs, parts, blobs, off = [], {}, [], 0
    for i in range(N_SRC):
        e, x = R.RefEncoder("fix", rate=13600), R.synth_stream(4100 + i, n_packets)
        recs.append([])
        for k in range(n_packets):
            pl, n0, n1 = e.encode(x[k])
            recs[i].append((pl, n0, n1))
            for d, part in enumerate((pl[:n0 - n1], pl[n0 - n1:n0])):
                parts[(i, k, d)] = (off, len(part))
                blobs.append(part)
                off += len(part)
    return recs, parts, np.frombuffer(b"".join(blobs), np.uint8).copy()


class RefSide:
    """the model's side of the tick: the ring model, the model of the rule, the compiled reference decoder and the time-scaling model"""

    def __init__(self, recs, parts, pool_bytes, p):
        self.recs, self.parts, self.pool_bytes, self.p = recs, parts, pool_bytes, p
        self.ring = RingModel(PL.E2E_NS, PL.E2E_DEPTH, 256)
        self.ring.track(True)
        self.rows = [PM.Row(640) for _ in range(PL.E2E_NS)]
        self.dec = [R.RefDecoder("fix", use_md_index=0) for _ in range(PL.E2E_NS)]

    def rows_of(self, arr):
        return [(s, k, d) + self.parts[(s % N_SRC, k, d)] for s, k, d in arr]

    def _decode(self, s, played):
        out = []
        for seq, (sa, sb) in played:
            pl, n0, n1 = self.recs[s % N_SRC][seq]
            x, ret = self.dec[s].decode(*R.map_loss(pl, n0, n1, sa is None, sb is None))
            assert ret == 0
            out.append(x)
        return np.stack(out)

    def tick(self, arr):
        ring, p = self.ring, self.p
        ring.insert(self.rows_of(arr), self.pool_bytes, [0] * PL.E2E_NS, {})
        rep = ring.report(None, clear_margin=True)[0]
        ls = list(range(PL.E2E_NS))
        pl = PM.plan(self.rows, ls, rep, p, PL.E2E_DEPTH)
        one = [self._decode(s, pk) for s, pk in zip(pl["one"], ring.play_out(pl["one"], 1))]
        two = [self._decode(s, pk) for s, pk in zip(pl["two"], ring.play_out(pl["two"], 2))]
        dec = dict(pcm_one=np.array([x[0] for x in one], np.int16).reshape(-1, 640), st_one=np.zeros(len(one), np.int32),
                   pcm_two=np.array(two, np.int16).reshape(-1, 2, 640), st_two=np.zeros(len(two), np.int32))
        if pl["stretch_pos"]:
            ts = model_timescale(dec["pcm_one"][pl["stretch_pos"]][:, None, :], 2, 16000)
            dec["ts_s"], dec["cost_s"] = ts["out"], ts["cost"]
        if two:
            ts = model_timescale(dec["pcm_two"], 1, 16000)
            dec["ts_a"], dec["cost_a"] = ts["out"], ts["cost"]
        return pl, PM.render(self.rows, ls, pl, p, **dec)


def _tick_run(torch, ticks, gate):
    import solo_amd
    p = dict(PL.E2E_PARAMS, cost_gate=gate)
    recs, parts, pool = _packets(PL.E2E_PACKETS)
    payload = torch.from_numpy(pool).cuda()
    ref = RefSide(recs, parts, len(pool), p)
    b = solo_amd.SoloBatch(PL.E2E_NS, rate=13600, encoder=False, decoder=True)
    b.recv_create(PL.E2E_DEPTH, 256, 0)
    b.recv_track(True)
    po = solo_amd.Playout(PL.E2E_NS, 640)
    seen = set()
    for t, arr in enumerate(PL.e2e_arrivals(ticks)):
        pl, (heard, outcome, status, count) = ref.tick(arr)
        if arr:
            b.recv_insert(torch.tensor(ref.rows_of(arr), dtype=torch.int32).cuda(), payload)
        g_heard, g_outcome, g_status, g_count = po.tick(b, **p)
        c = po.count(g_count)
        assert c == dict(plan=pl["count"], render=count), (t, c)
        assert np.array_equal(g_outcome.cpu().numpy(), outcome) and np.array_equal(g_status.cpu().numpy(), status), t
        bad = np.flatnonzero((g_heard.cpu().numpy() != heard).any(axis=1))
        assert len(bad) == 0, (t, bad.tolist(), outcome[bad].tolist())
        seen |= set(int(o) for o in outcome)
    blob = po.get_state().cpu().numpy()
    assert np.array_equal(blob[:, :128], PM.records(ref.rows)) and np.array_equal(blob[:, 128:].copy().view(np.int16), PM.held_store(ref.rows))
    assert np.array_equal(b.recv_report()[0].cpu().numpy(), PL.reports_i32(ref.ring.report()[0]))
    b.close()
    return seen


@need_ref
def test_gpu_tick_against_the_compiled_reference(torch_cuda):
    """12 streams at 13.6 kbps, ring depth 8, 64 ticks of the scripted network with the gate off: every outcome but the gated ones; then
    40 ticks with a gate of 1: both gated outcomes"""
    assert _tick_run(torch_cuda, PL.E2E_TICKS, 0) == set(range(8)) - {PM.O_STRETCH_GATED, PM.O_ACCEL_GATED}
    assert {PM.O_STRETCH_GATED, PM.O_ACCEL_GATED} <= _tick_run(torch_cuda, 40, 1)


def _encoded_pool(torch, n_packets):
    """the same kind of pool without the oracle: N_SRC streams encoded on the device"""
    import solo_amd
    pcm = np.stack([R.synth_stream(4100 + i, n_packets) for i in range(N_SRC)])
    e = solo_amd.SoloBatch(N_SRC, rate=13600, encoder=True, decoder=False)
    bits, nb, st = e.encode(torch.from_numpy(pcm).cuda())
    torch.cuda.synchronize()
    assert int(st.abs().max()) == 0
    hb, hn = bits.cpu().numpy(), nb.cpu().numpy()
    e.close()
    parts, blobs, off = {}, [], 0
    for i in range(N_SRC):
        for k in range(n_packets):
            n0, n1 = int(hn[i, k, 0]), int(hn[i, k, 1])
            pl = hb[i, k, :n0].tobytes()
            for d, part in enumerate((pl[:n0 - n1], pl[n0 - n1:])):
                parts[(i, k, d)] = (off, len(part))
                blobs.append(part)
                off += len(part)
    return parts, torch.from_numpy(np.frombuffer(b"".join(blobs), np.uint8).copy()).cuda()


def test_gpu_tick_equals_the_tick_by_hand(torch_cuda):
    """the same schedule on two handles: solo_playout_tick on one; on its twin recv_report, recv_decode(streams=) and timescale by hand,
    following the model's actions.  The same d_heard, tick for tick"""
    import solo_amd
    torch, p, ns, ticks = torch_cuda, PL.E2E_PARAMS, PL.E2E_NS, 56
    parts, payload = _encoded_pool(torch, PL.E2E_PACKETS)
    handles = []
    for _ in range(2):
        b = solo_amd.SoloBatch(ns, rate=13600, encoder=False, decoder=True)
        b.recv_create(PL.E2E_DEPTH, 256, 0)
        b.recv_track(True)
        handles.append(b)
    a, b = handles
    po, rows, ls, seen = solo_amd.Playout(ns, 640), [PM.Row(640) for _ in range(ns)], list(range(ns)), set()
    dev = lambda x: torch.tensor(x, dtype=torch.int32, device="cuda")
    for t, arr in enumerate(PL.e2e_arrivals(ticks)):
        if arr:
            d_arr = dev([(s, k, d) + parts[(s % N_SRC, k, d)] for s, k, d in arr])
            a.recv_insert(d_arr, payload)
            b.recv_insert(d_arr, payload)
        heard, outcome, status, count = po.tick(a, **p)
        rep = b.recv_report(clear_margin=True)[0].cpu().numpy().astype(np.int64)
        pl = PM.plan(rows, ls, rep, p, PL.E2E_DEPTH)
        dec = dict(pcm_one=np.zeros((0, 640), np.int16), st_one=np.zeros(0, np.int32), pcm_two=np.zeros((0, 2, 640), np.int16), st_two=np.zeros(0, np.int32))
        if pl["one"]:
            x, st = b.recv_decode(1, streams=dev(pl["one"]))
            dec["pcm_one"], dec["st_one"] = x[:, 0].cpu().numpy(), st.cpu().numpy()
            if pl["stretch_pos"]:
                cost = torch.zeros((len(pl["stretch_pos"]), 16), dtype=torch.int32, device="cuda")
                y, _ = b.timescale(x[dev(pl["stretch_pos"]).long()].contiguous(), 2, cost=cost)
                dec["ts_s"], dec["cost_s"] = y.cpu().numpy(), cost.cpu().numpy()
        if pl["two"]:
            x, st = b.recv_decode(2, streams=dev(pl["two"]))
            cost = torch.zeros((len(pl["two"]), 8), dtype=torch.int32, device="cuda")
            y, _ = b.timescale(x, 1, cost=cost)
            dec.update(pcm_two=x.cpu().numpy(), st_two=st.cpu().numpy(), ts_a=y.cpu().numpy(), cost_a=cost.cpu().numpy())
        want = PM.render(rows, ls, pl, p, **dec)
        assert np.array_equal(heard.cpu().numpy(), want[0]) and np.array_equal(outcome.cpu().numpy(), want[1]), t
        assert np.array_equal(status.cpu().numpy(), want[2]) and po.count(count) == dict(plan=pl["count"], render=want[3]), t
        seen |= set(int(o) for o in want[1])
    assert {PM.O_IDLE, PM.O_NORMAL, PM.O_HELD, PM.O_STRETCH, PM.O_ACCEL, PM.O_ACCEL_FORCED} <= seen
    assert np.array_equal(a.recv_report()[0].cpu().numpy(), b.recv_report()[0].cpu().numpy())       # both queues stand where they should
    a.close()
    b.close()


def _running_pair(torch, ticks=12):
    """a handle and its Playout after `ticks` ticks of the schedule"""
    import solo_amd
    parts, payload = _encoded_pool(torch, 24)
    b = solo_amd.SoloBatch(PL.E2E_NS, rate=13600, encoder=False, decoder=True)
    b.recv_create(PL.E2E_DEPTH, 256, 0)
    b.recv_track(True)
    po = solo_amd.Playout(PL.E2E_NS, 640)
    for arr in PL.e2e_arrivals(ticks, n_packets=24):
        if arr:
            b.recv_insert(torch.tensor([(s, k, d) + parts[(s % N_SRC, k, d)] for s, k, d in arr], dtype=torch.int32).cuda(), payload)
        po.tick(b, **PL.E2E_PARAMS)
    return b, po


def test_gpu_list_refusal_on_the_device_and_host_refusals(torch_cuda):
    """a list that is not increasing: nothing is written but n_one = -1; no state, queue or play position moves.  Then the host refusals of
    the tick: -1, nothing enqueued"""
    import solo_amd
    torch = torch_cuda
    b, po = _running_pair(torch)
    rep0, state0 = b.recv_report()[0].cpu().numpy(), po.get_state().cpu().numpy()
    assert (state0.view(np.int32)[:, 0] == 1).sum() >= 8
    prm = po.params(**PL.E2E_PARAMS)
    heard = torch.full((4, 640), PL.FILL_H, dtype=torch.int16, device="cuda")
    outc = torch.full((4,), PL.FILL_O, dtype=torch.int32, device="cuda")
    stat = torch.full((4,), PL.FILL_S, dtype=torch.int32, device="cuda")
    cnt = torch.full((12,), PL.FILL_N, dtype=torch.int32, device="cuda")

    def tick(obj=po.h, handle=b.h, rows=None, n=4, p=C.byref(prm), h=heard.data_ptr(), o=outc.data_ptr(), s=stat.data_ptr(), c=cnt.data_ptr()):
        return po.lib.solo_playout_tick(obj, handle, rows, n, p, h, o, s, c, po._stream())

    for bad in ([3, 3, 5, 7], [5, 3, 7, 9], [0, 1, 2, PL.E2E_NS], [-1, 0, 1, 2]):
        rows = torch.tensor(bad, dtype=torch.int32, device="cuda")
        assert tick(rows=rows.data_ptr()) == 0
        torch.cuda.synchronize()
        assert cnt.cpu().numpy().tolist() == [-1] + [PL.FILL_N] * 11
        assert bool((heard == PL.FILL_H).all()) and bool((outc == PL.FILL_O).all()) and bool((stat == PL.FILL_S).all())
        assert np.array_equal(po.get_state().cpu().numpy(), state0) and np.array_equal(b.recv_report()[0].cpu().numpy(), rep0)
        cnt[0] = PL.FILL_N
        h2, o2, s2, c2 = po.tick(b, streams=rows, **PL.E2E_PARAMS)                                # ... and through the binding
        assert po.count(c2)["plan"]["n_one"] == -1 and not bool(h2.any()) and not bool(o2.any()) and int(c2[1:].abs().sum()) == 0
        assert np.array_equal(po.get_state().cpu().numpy(), state0) and np.array_equal(b.recv_report()[0].cpu().numpy(), rep0)
    good = torch.tensor([1, 4, 6, 11], dtype=torch.int32, device="cuda")
    # the host refusals
    assert tick(obj=None) == -1 and tick(handle=None) == -1 and tick(p=None) == -1
    assert tick(h=None, rows=good.data_ptr()) == -1 and tick(o=None, rows=good.data_ptr()) == -1 and tick(s=None, rows=good.data_ptr()) == -1
    assert tick(c=None, rows=good.data_ptr()) == -1
    assert tick() == -1 and tick(n=0, rows=good.data_ptr()) == -1 and tick(n=PL.E2E_NS + 1, rows=good.data_ptr()) == -1    # NULL list with n != n_rows
    assert tick(h=heard.data_ptr() + 2, rows=good.data_ptr()) == -1 and tick(c=cnt.data_ptr() + 4, rows=good.data_ptr()) == -1
    bad_prm = solo_amd.solo_playout_params_t(2, 0, 40, 1, 1, 3, 8, 0)
    assert tick(p=C.byref(bad_prm), rows=good.data_ptr()) == -1
    no_ring = solo_amd.SoloBatch(PL.E2E_NS, encoder=False, decoder=True)
    assert tick(handle=no_ring.h, rows=good.data_ptr()) == -1                                     # a handle without a ring
    no_ring.recv_create(1, 256, 0)
    no_ring.recv_track(True)
    assert tick(handle=no_ring.h, rows=good.data_ptr()) == -1                                     # a ring of depth 1
    no_ring.recv_create(PL.E2E_DEPTH, 256, 0)
    no_ring.recv_track(False)
    assert tick(handle=no_ring.h, rows=good.data_ptr()) == -1                                     # tracking off
    no_ring.close()
    other_n = solo_amd.SoloBatch(PL.E2E_NS + 1, encoder=False, decoder=True)
    other_n.recv_create(PL.E2E_DEPTH, 256, 0)
    other_n.recv_track(True)
    assert tick(handle=other_n.h, rows=good.data_ptr()) == -1                                     # another stream count
    other_n.close()
    wb = solo_amd.SoloBatch(PL.E2E_NS, rate=24000, encoder=False, decoder=True, samplerate=32000)
    wb.recv_create(PL.E2E_DEPTH, 256, 0)
    wb.recv_track(True)
    assert tick(handle=wb.h, rows=good.data_ptr()) == -1                                          # another packet length
    wb.close()
    torch.cuda.synchronize()
    assert bool((cnt == PL.FILL_N).all()) and bool((heard == PL.FILL_H).all())
    assert np.array_equal(po.get_state().cpu().numpy(), state0) and np.array_equal(b.recv_report()[0].cpu().numpy(), rep0)
    assert tick(rows=good.data_ptr()) == 0                                                        # and the pair ticks on afterwards
    c = po.count(cnt)
    assert c["plan"]["listed"] == 4 and sum(c["render"].values()) == 4 and not bool((heard == PL.FILL_H).all())
    b.close()


def test_gpu_tick_on_a_side_stream_and_with_a_list(torch_cuda):
    """through the binding on a non-default stream: the listed streams tick, the others keep queue, play position and state"""
    torch = torch_cuda
    b, po = _running_pair(torch)
    twin_b, twin_po = _running_pair(torch)
    rep0, state0 = b.recv_report()[0].cpu().numpy(), po.get_state().cpu().numpy()
    listed = [0, 2, 3, 6, 7, 10]
    others = [s for s in range(PL.E2E_NS) if s not in listed]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        heard, outcome, status, count = po.tick(b, streams=listed, **PL.E2E_PARAMS)
        c = po.count(count)
    side.synchronize()
    full = twin_po.tick(twin_b, **PL.E2E_PARAMS)                                                   # the same tick with every stream, on the default stream
    torch.cuda.synchronize()
    assert c["plan"]["listed"] == len(listed) and sum(c["render"].values()) == len(listed)
    assert np.array_equal(heard.cpu().numpy(), full[0].cpu().numpy()[listed]) and np.array_equal(outcome.cpu().numpy(), full[1].cpu().numpy()[listed])
    assert bool(heard.any())
    rep1, state1 = b.recv_report()[0].cpu().numpy(), po.get_state().cpu().numpy()
    assert np.array_equal(state1[others], state0[others]) and np.array_equal(rep1[others][:, :15], rep0[others][:, :15])
    assert np.array_equal(state1[listed], twin_po.get_state().cpu().numpy()[listed]) and not np.array_equal(state1[listed], state0[listed])
    b.close()
    twin_b.close()

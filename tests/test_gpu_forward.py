"""Forwarding without transcoding on the GPU (solo_forward_levels / solo_forward_route through the C ABI) against the independent model of
tests/forward_model.py: the scenarios of tests/test_forward_model.py field for field after every tick -- A: 12 ticks at 24 rows in rooms of
1 .. 13 (the in-wave ranking of a room), B: one room of 700 (the walk over d_room, past 64 and 256 lanes; 699 records an arrival: the
emission's search crosses tiles) --, a room id refused on the device, the tick levels + select + route + egress pack captured in a graph
and replayed against eager twins, and the whole secured path end to end: three encoders' packets through ingest pack, protect, unprotect,
parse, the forwarding tick, egress pack and protect, a receiver's unprotect, parse, insert and decode, bit for bit against a twin that
was handed the source payloads under the packet numbers the model predicts.

CAPTURED names the test that captures each of the two calls the interface calls capturable (tests/test_forward_model.py holds this file
to it)."""
import ctypes as C

import numpy as np
import pytest

import forward_model as M
import graph_replay_lib as G

pytestmark = pytest.mark.gpu
CAPTURED = {"solo_forward_levels": "test_capture_forward_tick", "solo_forward_route": "test_capture_forward_tick"}
FILL8, FILL32 = 0xA5, -7


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(torch, t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def send_count_of(a):
    a = np.ascontiguousarray(a)
    return dict(records=int(a[0]), records_needed=int(a[1]), bytes=int(a[2:4].view(np.int64)[0]), bytes_needed=int(a[4:6].view(np.int64)[0]),
                empty=int(a[6]), refused=int(a[7]))


class GpuForward:
    """a solo_forward_t driven through the C ABI with guarded buffers; call() is what forward_model.run() drives"""

    def __init__(self, torch, n_rows, K):
        import solo_amd
        self.torch, self.n_rows, self.K = torch, n_rows, K
        self.f = solo_amd.Forward(n_rows, K)
        self.lib = self.f.lib

    def state(self):
        return np.ascontiguousarray(host(self.torch, self.f.get_state())).view(np.int32)

    def levels(self, tick, n):
        t = self.torch
        arr = dev(t, tick["arrivals"])
        lev = None if tick["level_in"] is None else dev(t, tick["level_in"])
        ri = t.full((n + 2, 4), FILL32, dtype=t.int32, device="cuda")
        sa, lv = t.full((n + 2,), FILL8, dtype=t.uint8, device="cuda"), t.full((n + 2,), FILL8, dtype=t.uint8, device="cuda")
        r = self.lib.solo_forward_levels(arr.data_ptr() or None, None if lev is None else lev.data_ptr(), arr.shape[0], n, tick["default_level"], ri.data_ptr(),
                                         sa.data_ptr(), lv.data_ptr(), self.f._stream())
        assert r == 0
        hri, hsa, hlv = host(t, ri), host(t, sa), host(t, lv)
        assert (hri[n:] == FILL32).all() and (hsa[n:] == FILL8).all() and (hlv[n:] == FILL8).all()
        return arr, ri, hri[:n], hsa[:n], hlv[:n]

    def route(self, arr, ri, tick, n, n_rooms, mr, guard=8):
        t = self.torch
        rec = t.full((mr + guard, 5), FILL32, dtype=t.int32, device="cuda")
        sc, cnt = t.full((8,), -9, dtype=t.int32, device="cuda"), t.full((8,), -9, dtype=t.int32, device="cuda")
        lf = t.full((n * self.K + guard,), FILL8, dtype=t.uint8, device="cuda")
        src = t.full((n_rooms + 1, self.K), FILL32, dtype=t.int32, device="cuda")
        sel, room = dev(t, tick["sel"]), dev(t, tick["room"])
        r = self.lib.solo_forward_route(self.f.h, arr.data_ptr() or None, arr.shape[0], ri.data_ptr(), sel.data_ptr(), room.data_ptr(), n, n_rooms, rec.data_ptr(), mr,
                                        sc.data_ptr(), lf.data_ptr(), src.data_ptr(), cnt.data_ptr(), self.f._stream())
        assert r == 0
        return host(t, rec), host(t, sc), host(t, cnt), host(t, lf), host(t, src)

    def call(self, n, n_rooms):
        def go(tick, _words, mr):
            arr, ri, hri, hsa, hlv = self.levels(tick, n)
            rec, sc, cnt, lf, src = self.route(arr, ri, tick, n, n_rooms, mr)
            assert (lf[n * self.K:] == FILL8).all() and (src[n_rooms:] == FILL32).all()
            return dict(rowinfo=hri, sa=hsa, level=hlv, records=rec, send_count=send_count_of(sc), count=dict(zip(M.COUNT_FIELDS, (int(v) for v in cnt))),
                        level_fwd=lf[:n * self.K].astype(np.int64), slot_src=src[:n_rooms], state=self.state(), fill32=FILL32, fill8=FILL8)
        return go


# ---- the scenarios -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 3])
def test_scenario_a(torch_cuda, K):
    n, n_rooms = M.A_ROWS, M.A_ROOMS
    ticks = M.scenario_a(100 + K, K)
    g, model = GpuForward(torch_cuda, n, K), M.Forward(n, K)
    results = M.run(model, ticks, n, n_rooms, g.call(n, n_rooms))
    total = {k: sum(r["count"][k] for r in results) for k in M.COUNT_FIELDS}
    print("scenario A, K = %d: %s" % (K, total))
    assert all(total[k] > 0 for k in M.COUNT_FIELDS), total
    # the arrivals of every tick in another order: the same state, counts and per-row outputs, the same records as a multiset
    rng = np.random.default_rng(7)
    g2, model2 = GpuForward(torch_cuda, n, K), M.Forward(n, K)
    again = M.run(model2, [M.permuted(t, rng) for t in ticks], n, n_rooms, g2.call(n, n_rooms), cut_all=True)
    for a, b in zip(results, again):
        assert a["count"] == b["count"] and a["slot_src"] == b["slot_src"] and a["level_fwd"] == b["level_fwd"]
        assert sorted(a["records"]) == sorted(b["records"])
    assert np.array_equal(g.state(), g2.state())


def test_scenario_b(torch_cuda):
    n, K = M.B_ROWS, 3
    ticks = M.scenario_b(5)
    g, model = GpuForward(torch_cuda, n, K), M.Forward(n, K)
    results = M.run(model, ticks, n, 1, g.call(n, 1))
    print("scenario B: %s" % [r["count"] for r in results])
    assert all(r["count"]["forwarded"] > 0 and len(r["records"]) == 699 * r["count"]["forwarded"] for r in results)
    rng = np.random.default_rng(8)
    g2, model2 = GpuForward(torch_cuda, n, K), M.Forward(n, K)
    again = M.run(model2, [M.permuted(t, rng) for t in ticks], n, 1, g2.call(n, 1), cut_all=True)
    assert all(sorted(a["records"]) == sorted(b["records"]) and a["count"] == b["count"] for a, b in zip(results, again))
    assert np.array_equal(g.state(), g2.state())


def test_state_calls_and_listed_reset(torch_cuda):
    """get_state / set_state / reset_rooms of the row object under it: a state that travels to a second object continues the scenario"""
    torch = torch_cuda
    n, K = M.A_ROWS, 3
    ticks = M.scenario_a(3, K)
    g, model = GpuForward(torch, n, K), M.Forward(n, K)
    assert np.array_equal(g.state(), model.state())                 # what create leaves: {-1, 0, 0, 0} in every slot
    M.run(model, ticks[:4], n, M.A_ROOMS, g.call(n, M.A_ROOMS))
    before = g.state()
    for lst in ([n], [-1], [2, 2]):
        a = (C.c_int32 * len(lst))(*lst)
        assert g.lib.solo_forward_reset_rooms(g.f.h, a, len(lst), g.f._stream()) == -1
    assert g.lib.solo_forward_reset_rooms(g.f.h, None, 1, g.f._stream()) == -1 and np.array_equal(g.state(), before)
    g.f.reset([4, 1])
    model.reset([4, 1])
    assert np.array_equal(g.state(), model.state()) and g.state()[4].tolist() == [-1, 0, 0, 0] * K
    g2 = GpuForward(torch, n, K)
    rooms = dev(torch, np.array([3, 2, 0], np.int32))
    blob = g.f.get_state(rooms)
    assert np.array_equal(np.ascontiguousarray(host(torch, blob)).view(np.int32), model.state()[[3, 2, 0]])
    g2.f.set_state(blob, rooms)
    g2.f.set_state(g.f.get_state(dev(torch, np.array([1, 4], np.int32))), dev(torch, np.array([1, 4], np.int32)))
    assert np.array_equal(g2.state(), model.state())
    M.run(model, ticks[4:], n, M.A_ROOMS, g2.call(n, M.A_ROOMS))
    g2.f.reset()
    assert np.array_equal(g2.state(), M.Forward(n, K).state())
    assert g.lib.solo_forward_create(0, 2) is None and g.lib.solo_forward_create(4, 0) is None and g.lib.solo_forward_create(4, 9) is None


def test_room_id_refused_on_the_device(torch_cuda):
    n, K = M.A_ROWS, 2
    ticks = M.scenario_a(4, K)
    g, model = GpuForward(torch_cuda, n, K), M.Forward(n, K)
    M.run(model, ticks[:3], n, M.A_ROOMS, g.call(n, M.A_ROOMS))
    before = g.state()
    for bad in (-2, M.A_ROOMS):
        tick = dict(ticks[3], room=ticks[3]["room"].copy())
        tick["room"][9] = bad
        arr, ri, _, _, _ = g.levels(tick, n)
        rec, sc, cnt, lf, src = g.route(arr, ri, tick, n, M.A_ROOMS, 50)
        assert cnt[0] == -1 and sc[0] == -1 and (cnt[1:] == -9).all() and (sc[1:] == -9).all()
        assert (rec == FILL32).all() and (lf == FILL8).all() and (src == FILL32).all() and np.array_equal(g.state(), before)
    M.run(model, ticks[3:5], n, M.A_ROOMS, g.call(n, M.A_ROOMS))    # ... and the object goes on as if the call had not been made


def test_argument_rules_of_the_library(torch_cuda):
    """-1 with nothing enqueued (the rules themselves: tests/test_forward_model.py, on the same two functions)"""
    torch = torch_cuda
    n, K = 8, 2
    g = GpuForward(torch, n, K)
    arr, ri = dev(torch, np.zeros((4, 5), np.int32)), torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    sa, lv = torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
    s = g.f._stream()
    ok = [arr.data_ptr(), None, 4, n, 255, ri.data_ptr(), sa.data_ptr(), lv.data_ptr(), s]
    assert g.lib.solo_forward_levels(*ok) == 0
    for at, v in ((5, None), (6, None), (7, None), (2, -1), (0, None), (3, 0), (4, 256), (5, ri.data_ptr() + 2), (0, arr.data_ptr() + 1)):
        bad = list(ok)
        bad[at] = v
        assert g.lib.solo_forward_levels(*bad) == -1, (at, v)
    sel, room = torch.ones(n, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    rec, sc, cnt = torch.zeros((64, 5), dtype=torch.int32, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda"), torch.zeros(8, dtype=torch.int32, device="cuda")
    ok = [g.f.h, arr.data_ptr(), 4, ri.data_ptr(), sel.data_ptr(), room.data_ptr(), n, 1, rec.data_ptr(), 64, sc.data_ptr(), None, None, cnt.data_ptr(), s]
    state = g.state()
    for at, v in ((0, None), (3, None), (4, None), (5, None), (8, None), (10, None), (13, None), (6, 0), (6, n + 1), (7, 0), (7, n + 1), (2, -1), (1, None),
                  (9, -1), (2, 2 ** 31 // (n - 1) + 1), (8, rec.data_ptr() + 2), (10, sc.data_ptr() + 4)):
        bad = list(ok)
        bad[at] = v
        assert g.lib.solo_forward_route(*bad) == -1, (at, v)
    assert np.array_equal(g.state(), state)
    assert g.lib.solo_forward_route(*ok) == 0
    torch.cuda.synchronize()


def test_forward_kernels_use_no_private_memory():
    """the metadata check of tests/test_forward_model.py, on the library the GPU tests run"""
    from test_forward_model import test_forward_kernels_use_no_scratch as check
    check()


# ---- the tick in a graph ------------------------------------------------------------------------------------------------------------------------
def _graph_feeds(rng, n, nd, pool_bytes, k):
    """one tick of n rows in two rooms, padded to nd arrivals with what a parse rejected"""
    room = np.array([[0, 0, 1, 0, 1, 1, 0, -1], [0, 1, 1, 0, 1, -1, 0, 0], [1, 0, 1, 0, 1, 1, 0, 0], [0, 0, 1, 1, 1, 1, -1, 0], [0, 0, 0, 1, 1, 1, 1, 0]][k], np.int32)
    arr, lev = [], []
    for x in range(n):
        for j in range(int(rng.integers(0, 3))):
            for d in (0, 1):
                ln = int(rng.integers(1, 120))
                arr.append((x, 100 * x + 2 * k + j, d, int(rng.integers(0, pool_bytes - ln)), ln))
                lev.append(int(rng.integers(0, 100)) | (128 if rng.integers(0, 3) else 0))
    assert len(arr) <= nd
    while len(arr) < nd:
        arr.append((-1, 0, 0, 0, 0))
        lev.append(255)
    order = rng.permutation(nd)
    return dict(arrivals=np.array([arr[i] for i in order], np.int32), level_in=np.array([lev[i] for i in order], np.uint8), room=room)


def test_capture_forward_tick(torch_cuda):
    """levels + select + route + the egress pack in ONE graph, n_dgrams, n and max_records frozen; arrivals, levels and room ids move
    between replays; every output and the state of Forward and Vad against twins that make the same calls eagerly, and the records and
    counts against the model"""
    import solo_amd
    torch = torch_cuda
    n, K, ND, MAXR, POOL, CAP = 8, 2, 40, 96, 4096, 1 << 15
    rng = np.random.default_rng(21)
    pool = rng.integers(0, 256, POOL, dtype=np.uint8)
    prm = dict(max_speakers=K, on=128, off=64, hang=0, stick=6)

    def make():
        f, v, eg = solo_amd.Forward(n, K), solo_amd.Vad(n, 320), solo_amd.Rtp(n * K, 640)
        eg.bind(list(range(n * K)), [7000 + i for i in range(n * K)], 11, 22, (96, 97), 3)
        d_pool = dev(torch, pool)
        ins = dict(arrivals=G.zeros(torch, (ND, 5), torch.int32), level_in=G.zeros(torch, (ND,), torch.uint8), room=G.zeros(torch, (n,), torch.int32))
        outs = dict(rowinfo=G.zeros(torch, (n, 4), torch.int32), sa=G.zeros(torch, (n,), torch.uint8), level=G.zeros(torch, (n,), torch.uint8),
                    sel=G.zeros(torch, (n, 1), torch.uint8), vcount=G.zeros(torch, (4,), torch.int32), records=G.zeros(torch, (MAXR, 5), torch.int32),
                    send_count=G.zeros(torch, (8,), torch.int32), level_fwd=G.zeros(torch, (n * K,), torch.uint8), slot_src=G.zeros(torch, (2, K), torch.int32),
                    count=G.zeros(torch, (8,), torch.int32), dgrams=G.zeros(torch, (MAXR, 2), torch.int32), wire=G.zeros(torch, (CAP,), torch.uint8),
                    pcount=G.zeros(torch, (8,), torch.int32))
        p = solo_amd.solo_vad_select_params_t(prm["max_speakers"], prm["on"], prm["off"], prm["hang"], prm["stick"])

        def call():
            s, L = f._stream(), f.lib
            return (L.solo_forward_levels(ins["arrivals"].data_ptr(), ins["level_in"].data_ptr(), ND, n, 255, outs["rowinfo"].data_ptr(), outs["sa"].data_ptr(),
                                          outs["level"].data_ptr(), s) or
                    L.solo_vad_select(v.h, None, n, outs["sa"].data_ptr(), outs["level"].data_ptr(), 1, 1, ins["room"].data_ptr(), 2, C.byref(p), None,
                                      outs["sel"].data_ptr(), None, None, None, outs["vcount"].data_ptr(), s) or
                    L.solo_forward_route(f.h, ins["arrivals"].data_ptr(), ND, outs["rowinfo"].data_ptr(), outs["sel"].data_ptr(), ins["room"].data_ptr(), n, 2,
                                         outs["records"].data_ptr(), MAXR, outs["send_count"].data_ptr(), outs["level_fwd"].data_ptr(), outs["slot_src"].data_ptr(),
                                         outs["count"].data_ptr(), s) or
                    L.solo_rtp_pack(eg.h, outs["records"].data_ptr(), outs["send_count"].data_ptr(), MAXR, d_pool.data_ptr(), POOL, outs["level_fwd"].data_ptr(), 1,
                                    outs["dgrams"].data_ptr(), outs["wire"].data_ptr(), CAP, outs["pcount"].data_ptr(), s))
        state = lambda: np.concatenate([host(torch, f.get_state()).reshape(-1), host(torch, v.get_state()).reshape(-1)])
        return G.Stage(torch, ins, outs, call, state=state, keep=(f, v, eg, d_pool, p))

    fm = M.Forward(n, K)
    seen = dict(switches=0, forwarded=0)

    def model(k, feed, got):
        rows = M.levels(feed["arrivals"], feed["level_in"], n, 255)
        assert np.array_equal(got["rowinfo"], M.rowinfo_words(rows)), k
        res = fm.route(feed["arrivals"], rows, got["sel"][:, 0], feed["room"], n, 2)
        want_rec, want_send = M.cut(res, MAXR)
        cnt = dict(zip(M.COUNT_FIELDS, (int(x) for x in got["count"])))
        assert cnt == res["count"] and send_count_of(got["send_count"]) == want_send, (k, cnt, res["count"])
        assert np.array_equal(got["records"][:want_send["records"]], want_rec) and got["slot_src"].tolist() == res["slot_src"], k
        assert int(got["pcount"][0]) == want_send["records"], k     # every record became a datagram
        seen["switches"] += cnt["switches"]
        seen["forwarded"] += cnt["forwarded"]

    feeds = [_graph_feeds(rng, n, ND, POOL, k) for k in range(5)]
    _, cap, _ = G.replay_against_twin(torch, make, feeds, model=model, stateful=True)
    assert np.array_equal(np.ascontiguousarray(host(torch, cap.keep[0].get_state())).view(np.int32), fm.state())
    assert seen["switches"] >= 4 and seen["forwarded"] >= 10, seen


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------------
def test_end_to_end_secured_forwarding(torch_cuda):
    """4 rows in one room, K = 2, 8 packets at 16 kHz, one tick a packet.  Rows 0 .. 2 send (three encoders; row 3 only listens): ingest pack
    and protect (the senders), then per tick on the server unprotect, parse, levels, select, route, egress pack and protect with no host
    loop over datagrams; the receiver of row 3 runs unprotect, parse, solo_recv_insert over what the egress wrote and decodes its two slot
    streams.  The voiced rows are 0 and 1 for four packets, then 1 and 2: slot 0 changes its speaker in mid-stream and stays continuous.
    The PCM equals, bit for bit, that of a twin handle which was given the same source payloads directly under the packet numbers the
    model predicts."""
    import solo_amd
    import test_gpu_rtp as R
    torch = torch_cuda
    rng = np.random.default_rng(77)
    N, K, P, L, FIRST = 4, 2, 8, 640, 500
    bits, nb, md = R._encoded(torch, 3, P, 16000)
    assert md == [0, 0, 0]
    base = rng.integers(0, 1000, 3).astype(np.int32)
    first = [FIRST + int(b) for b in base]
    tx = solo_amd.SoloBatch(3, encoder=True, decoder=False)
    records, payload, scount = tx.send_pack(bits, nb, first_seq=FIRST, seq_base=dev(torch, base))
    n_rec = 2 * 3 * P
    assert tx.send_count(scount)["records"] == n_rec

    def session(n_streams, ssrc0, offsets, masters, tx_keys):
        r = solo_amd.Rtp(n_streams, L)
        r.bind(list(range(n_streams)), [ssrc0 + 17 * i for i in range(n_streams)], offsets[0], offsets[1], (96, 97), 3)
        if tx_keys:
            r.set_trailer(10)
        r.set_keys(list(range(n_streams)), tx=masters if tx_keys else None, rx=masters)
        return r
    offsets = lambda k: ([int(v) for v in rng.integers(0, 2 ** 32, k)], [int(v) for v in rng.integers(0, 2 ** 16, k)])
    m_in, m_out = rng.integers(0, 256, (N, 30), dtype=np.uint8), rng.integers(0, 256, (N * K, 30), dtype=np.uint8)
    off_in, off_out = offsets(N), offsets(N * K)
    ing, eg = session(N, 1000, off_in, m_in, True), session(N * K, 5000, off_out, m_out, True)
    rcv = session(N * K, 5000, off_out, m_out, False)               # the receiver's session: the egress SSRCs, offsets and keys
    # the senders: a level byte per packet (voiced: rows 0 and 1, then 1 and 2), pack, protect
    level = np.zeros((N, P), np.uint8)
    for s in range(3):
        for pk in range(P):
            voiced = s in ((0, 1) if pk < 4 else (1, 2))
            level[s, (first[s] + pk) % P] = (0x80 | (20 + s)) if voiced else 90
    dgrams, wire, _ = ing.pack(records, scount, payload, level=dev(torch, level))
    assert ing.srtp_count(ing.protect(records, scount, dgrams, wire))["ok"] == n_rec
    rec, dg = host(torch, records)[:n_rec], host(torch, dgrams)[:n_rec]
    orig = {(int(s), int(q), int(d)): int(off) for s, q, d, off, _ in rec}
    # the server and the receiver
    ringb = R.ring_handle(N, first + [0], depth=P)
    fwd, vad, fm = solo_amd.Forward(N, K), solo_amd.Vad(N, 320), M.Forward(N, K)
    room_np = np.zeros(N, np.int32)
    room = dev(torch, room_np)
    rxh = R.ring_handle(N * K, [0] * (N * K), depth=P)
    twin_rows, total, switches = [], 0, 0
    for pk in range(P):
        idx = np.array([i for i in range(n_rec) if rec[i, 1] - first[rec[i, 0]] == pk])
        idx = idx[rng.permutation(len(idx))]
        out, ucnt = ing.unprotect(dev(torch, dg[idx]), wire)
        arr, lv, _, pcnt = ing.parse(ringb, out, wire, level=True)
        lvl = fwd.levels(arr, lv)
        sel = vad.select(lvl["sa"][:, None, None], lvl["level"][:, None], room, n_rooms=1, max_speakers=K, hang=0)["sel"]
        r = fwd.route(arr, lvl["rowinfo"], sel, room, n_rooms=1)
        dg2, wire2, _ = eg.pack(r["records"], r["send_count"], wire, level=r["level_fwd"])
        pcount = eg.protect(r["records"], r["send_count"], dg2, wire2)
        # what the model says of this tick
        ha = host(torch, arr)
        assert ing.srtp_count(ucnt)["ok"] == len(idx) == ing.parse_count(pcnt)["accepted"] == ing.parse_count(pcnt)["with_level"]
        rows = M.levels(ha, host(torch, lv), N, 255)
        assert np.array_equal(host(torch, lvl["rowinfo"]), M.rowinfo_words(rows))
        res = fm.route(ha, rows, host(torch, sel)[:, 0], room_np, N, 1)
        want_rec, want_send = M.cut(res, len(res["records"]))
        assert fwd.count(r["count"]) == res["count"] and send_count_of(host(torch, r["send_count"])) == want_send
        nr = want_send["records"]
        assert nr == 3 * 2 * 2 and np.array_equal(host(torch, r["records"])[:nr], want_rec) and eg.srtp_count(pcount)["ok"] == nr
        assert [rows[x]["sa"] for x in range(N)] == [255 * int(x in ((0, 1) if pk < 4 else (1, 2))) for x in range(N)]
        total += nr
        switches += res["count"]["switches"]
        for (s, q, d, _, _), mine in zip(ha.tolist(), res["per_arrival"]):
            twin_rows += [(st, pn, dd, orig[s, q, d], ln) for st, pn, dd, _, ln in mine if st // K == 3]
        # the receiver: every datagram the egress wrote
        out2, ucnt2 = rcv.unprotect(dg2[:nr], wire2)
        arr2, _, _, pcnt2 = rcv.parse(rxh, out2, wire2)
        assert rcv.srtp_count(ucnt2)["ok"] == nr == rcv.parse_count(pcnt2)["accepted"]
        rxh.recv_insert(arr2, wire2)
    assert switches == 3 and rxh.recv_stats() == dict(inserted=total, late=0, ahead=0, duplicate=0, bad=0)
    mine = [3 * K, 3 * K + 1]
    assert sorted({(st, pn) for st, pn, _, _, _ in twin_rows}) == [(st, pn) for st in mine for pn in range(P)]      # both slots continuous, 0 .. 7
    got, st = rxh.recv_decode(P, streams=mine)
    twin = R.ring_handle(N * K, [0] * (N * K), depth=P)
    twin.recv_insert(dev(torch, np.array(twin_rows, np.int32)), payload)
    assert twin.recv_stats() == dict(inserted=len(twin_rows), late=0, ahead=0, duplicate=0, bad=0)
    want, wst = twin.recv_decode(P, streams=mine)
    got, st = host(torch, got), host(torch, st)
    assert np.array_equal(got, host(torch, want)) and np.array_equal(st, host(torch, wst))
    assert got.shape == (2, P, L) and got[0].any() and got[1].any()
    for o in (ing, eg, rcv, fwd):
        o.close()

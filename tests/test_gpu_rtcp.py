"""RTCP on the GPU (solo_rtcp_* through the C ABI and through solo_amd.Rtcp) against the independent model of tests/rtcp_model.py: the
scenarios of tests/test_rtcp_model.py state word for state word, wire byte for wire byte and count for count after every tick, at 8 and
at 70 streams (one wavefront of streams plus six) -- (a) clean, (b) loss, reordering and duplicates, (c) a sequence cycle and a clock
that crosses 2^32, (d) jumps of 2999 / 3000 / 3001 with the resynchronisation and a misorder of 99 / 100 / 101, (e) one stream with
RTCP_WALK_MAX - 1, RTCP_WALK_MAX, RTCP_WALK_MAX + 1 and 300 datagrams in a call beside an empty call, rejected arrivals and desc = -1,
(f) the clamp of the cumulative loss, (g) the loopback of two sides with its round-trip time and the rejected packets --, the cap of
build, the independence of the order, one stream that owns a whole call, and the calls captured in graphs and replayed against eager twins.

CAPTURED names the test that captures each of the four calls the interface calls capturable (tests/test_rtcp_model.py holds this file
to it)."""
import ctypes as C
import random

import numpy as np
import pytest

import graph_replay_lib as G
import rtcp_model as M

pytestmark = pytest.mark.gpu
CAPTURED = {"solo_rtcp_received": "test_capture_received_tick", "solo_rtcp_sent": "test_capture_sent_tick",
            "solo_rtcp_build": "test_capture_build_and_parse", "solo_rtcp_parse": "test_capture_build_and_parse"}
FILL8, FILL32 = 0xA5, -7
L = 640


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch


def dev(torch, a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).cuda()


def host(torch, t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def check(ok, msg):
    assert ok, msg


def count_of(fields, a):
    return dict(zip(fields, (int(v) for v in a)))


def build_count_of(a):
    a = np.ascontiguousarray(a)
    return dict(built=int(a[0]), built_needed=int(a[1]), bytes=int(a[2:4].view(np.int64)[0]), bytes_needed=int(a[4:6].view(np.int64)[0]),
                refused=int(a[6]), with_sr=int(a[7]))


_sessions = {}


def gpu_session(ses):
    """a solo_amd.Rtp bound as the model's Session says (kept: a scenario asks for it every tick)"""
    import solo_amd
    key = (id(ses), tuple(ses.bound))
    if key not in _sessions:
        r = solo_amd.Rtp(ses.n, ses.L)
        s = [k for k in range(ses.n) if ses.bound[k]]
        r.bind(s, [ses.ssrc[k] for k in s], [ses.ts_offset[k] for k in s], 0, (96, 97), 0)
        _sessions[key] = (r, ses)
    return _sessions[key][0]


class GpuRtcp:
    """a solo_rtcp_t driven through the C ABI with guarded buffers, with the interface the drivers of tests/rtcp_model.py call"""

    def __init__(self, torch, n):
        import solo_amd
        self.torch, self.n = torch, n
        self.o = solo_amd.Rtcp(n)
        self.lib, self.h = self.o.lib, self.o.h

    def full(self, shape, v, dtype):
        return self.torch.full(shape, v, dtype=dtype, device="cuda")

    def words(self):
        return np.ascontiguousarray(host(self.torch, self.o.get_state())).view(np.uint32)

    def set_words(self, w):
        self.o.set_state(dev(self.torch, np.ascontiguousarray(w, np.uint32).view(np.uint8).reshape(self.n, 160)))

    def set_cname(self, streams, names):
        idx = (C.c_int32 * len(streams))(*streams)
        buf = b"".join(bytes(x).ljust(32, b"\0")[:32] for x in names)
        return self.lib.solo_rtcp_set_cname(self.h, idx if len(streams) else None, len(streams), buf, self.o._stream())

    def now(self, now, device_now):
        if not device_now:
            return now, None, None
        t = dev(self.torch, np.array([now], np.uint64).view(np.int64))
        return 0xDEADBEEF, t.data_ptr(), t

    def received(self, session, tick):
        t = self.torch
        arr, seq = dev(t, tick["arrivals"]), dev(t, tick["rtp_seq"].view(np.int16))
        at = None if tick["arrival_time"] is None else dev(t, tick["arrival_time"].view(np.int32))
        cnt = self.full((12,), FILL32, t.int32)
        r = self.lib.solo_rtcp_received(self.h, gpu_session(session).h, arr.data_ptr() or None, seq.data_ptr() or None, arr.shape[0],
                                        None if at is None else at.data_ptr(), tick["now_rtp"], cnt.data_ptr(), self.o._stream())
        cnt = host(t, cnt)
        assert r == 0 and (cnt[8:] == FILL32).all() and cnt[7] == 0
        return count_of(M.RECEIVED_COUNT, cnt)

    def sent(self, session, rec, n_rec, dg):
        t = self.torch
        sc, cnt = dev(t, np.array([n_rec, n_rec, 0, 0, 0, 0, 0, 0], np.int32)), self.full((12,), FILL32, t.int32)
        drec, ddg = dev(t, rec), dev(t, dg)
        r = self.lib.solo_rtcp_sent(self.h, gpu_session(session).h, drec.data_ptr(), sc.data_ptr(), rec.shape[0], ddg.data_ptr(), cnt.data_ptr(), self.o._stream())
        cnt = host(t, cnt)
        assert r == 0 and (cnt[8:] == FILL32).all() and (cnt[2:8] == 0).all()
        return count_of(M.SENT_COUNT, cnt)

    def build(self, tx, rx, streams, now, cap, guard=64, device_now=False):
        t = self.torch
        idx = dev(t, np.asarray(streams, np.int32))
        room = int(min(cap, 96 * len(streams)))
        dg, wire, cnt = self.full((len(streams) + 2, 2), FILL32, t.int32), self.full((room + guard,), FILL8, t.uint8), self.full((12,), FILL32, t.int32)
        now, p_now, keep = self.now(now, device_now)
        r = self.lib.solo_rtcp_build(self.h, gpu_session(tx).h, None if rx is None else gpu_session(rx).h, idx.data_ptr(), len(streams), now, p_now, dg.data_ptr(),
                                     wire.data_ptr(), cap, cnt.data_ptr(), self.o._stream())
        assert r == 0
        dg, wire, cnt = host(t, dg), host(t, wire), host(t, cnt)
        assert (cnt[8:] == FILL32).all() and (dg[len(streams):] == FILL32).all() and (wire[room:] == FILL8).all()
        if cnt[0] == -1:
            assert (dg == FILL32).all() and (wire == FILL8).all() and (cnt[1:] == FILL32).all()
            return 1, dg[:len(streams)], wire, dict(built=-1)
        c = build_count_of(cnt)
        assert (wire[c["bytes"]:] == FILL8).all()               # nothing at or beyond what was written, the cap included
        return 0, dg[:len(streams)], wire, c

    def parse(self, rx, tx, dgrams, wire, now, device_now=False):
        t = self.torch
        fb, cnt = self.full((self.n + 1, 8), 0x25A5A5A5, t.int32), self.full((20,), FILL32, t.int32)
        ddg, dw = dev(t, dgrams), dev(t, wire)
        now, p_now, keep = self.now(now, device_now)
        r = self.lib.solo_rtcp_parse(self.h, gpu_session(rx).h, None if tx is None else gpu_session(tx).h, ddg.data_ptr() or None, dgrams.shape[0],
                                     dw.data_ptr() or None, wire.shape[0], now, p_now, fb.data_ptr(), cnt.data_ptr(), self.o._stream())
        fb, cnt = host(t, fb), host(t, cnt)
        assert r == 0 and (cnt[16:] == FILL32).all() and (cnt[10:16] == 0).all() and (fb[self.n] == 0x25A5A5A5).all()
        return fb[:self.n].view(np.uint32).copy(), count_of(M.PARSE_COUNT, cnt)


def sessions(n):
    X = M.Session([0x10000000 + (s * 2654435761) % 0xFFFFF for s in range(n)], [(0xFFFFF000 + 977 * s) & M.M32 for s in range(n)], packet_samples=L)
    Y = M.Session([0xE0000000 - 31 * s * s - s for s in range(n)], [12345 * s for s in range(n)], packet_samples=L)
    return X, Y


def fresh(torch, n):
    impl, model = GpuRtcp(torch, n), M.Model(n)
    cn = [b"s%d@example.net" % s for s in range(n)]
    assert impl.set_cname(list(range(n)), cn) == 0
    model.set_cname(list(range(n)), cn)
    return impl, model


# ---- the scenarios -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 70])
@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e"])
def test_received_scenarios(torch_cuda, name, n):
    import solo_amd
    X, Y = sessions(n)
    impl, model = fresh(torch_cuda, n)
    offs = [65530] * n if name == "c" else [(7919 * s) & 0xFFFF for s in range(n)]
    ticks = M.scenario(name, n, 32, 11 + n, Y, offs, walk_max=solo_amd.RTCP_WALK_MAX)
    M.run_received(impl, model, Y, ticks, check)
    if name == "c":
        assert all(r["cycles"] == 65536 for r in model.rows)
    if name == "e":
        assert model.rows[3 % n]["received"] > 300 and max(len(t["arrivals"]) for t in ticks) > 300 and min(len(t["arrivals"]) for t in ticks) == 0


def test_duplicates_report_fraction_zero_and_the_clamp(torch_cuda):
    """(b) a negative interval loss reports fraction 0; (f) the cumulative loss driven past 24 bits through set_state is clamped, both ways"""
    n = 4
    X, Y = sessions(n)
    impl, model = fresh(torch_cuda, n)
    items = [(0, q, 0, 10 + q, 0) for q in range(5)] + [(0, 4, 0, 14, 0)] * 3
    M.run_received(impl, model, Y, [M.make_tick(items, False, 7)], check)
    w = model.words()
    w[1, :10] = (0, 100, 0x01000000, 65537, 5, 0, 0, 0, 0, 3)
    w[2, :10] = (0, 100, 0, 65537, 0x00900000, 0, 0, 0, 0, 3)
    model.set_words(w)
    impl.set_words(w)
    md, mw = M.both_build(impl, model, X, Y, [0, 1, 2], 99, 1 << 20, check, "clamp")
    blocks = [mw[o + 8 + 4:o + 8 + 8] for o, _ in md]
    assert blocks[0] == b"\x00\xff\xff\xfd" and blocks[1] == b"\xff\x7f\xff\xff" and blocks[2] == b"\x00\x80\x00\x00"


@pytest.mark.parametrize("n", [8, 70])
def test_sent_and_build_with_caps(torch_cuda, n):
    """sent() over records of every kind, then build() for changing lists: without and with report blocks, refused streams, a cap of 0,
    one byte short of the last packet and exact, and lists the device refuses"""
    X, Y = sessions(n)
    X.bound[2] = 0
    impl, model = fresh(torch_cuda, n)
    model.reset_rows([5])
    impl.o.reset([5])
    M.run_received(impl, model, Y, M.scenario("b", n, 4, 3, Y, [5] * n), check)
    Y.bound[n - 1] = 0
    M.run_sent_build(impl, model, X, Y, check)


@pytest.mark.parametrize("n,device_now", [(8, False), (70, True)])
def test_loopback(torch_cuda, n, device_now):
    X, Y = sessions(n)
    A, mA = fresh(torch_cuda, n)
    B, mB = fresh(torch_cuda, n)
    M.run_received(A, mA, Y, M.scenario("b", n, 3, 1, Y, [9] * n), check)
    M.run_received(B, mB, X, M.scenario("a", n, 3, 2, X, [65000] * n), check)
    rec = np.array([(s, 10 + k, k & 1, 0, 33 + s) for k in range(3) for s in range(n)], np.int32)
    dg = np.array([(0, 45 + s) for k in range(3) for s in range(n)], np.int32)
    for side, model, sess in ((A, mA, X), (B, mB, Y)):
        assert side.sent(sess, rec, len(rec), dg) == model.sent(rec, len(rec), dg)
    M.run_loopback(A, mA, B, mB, X, Y, check, now_kw=dict(device_now=True) if device_now else None)


def test_order_independence(torch_cuda):
    """sent and parse: any order of the inputs; received: any interleaving that keeps every stream's own order"""
    n = 70
    X, Y = sessions(n)
    rng = random.Random(8)
    ticks = M.scenario("b", n, 6, 21, Y, [65500] * n)
    ref, _ = fresh(torch_cuda, n)
    other, _ = fresh(torch_cuda, n)
    for tick in ticks:
        ref.received(Y, tick)
        per = [[i for i in range(len(tick["arrivals"])) if tick["arrivals"][i][0] == s] for s in range(n)]
        order = M.interleave(rng, per)
        other.received(Y, dict(arrivals=tick["arrivals"][order].copy(), rtp_seq=tick["rtp_seq"][order].copy(), arrival_time=tick["arrival_time"][order].copy(),
                               now_rtp=tick["now_rtp"]))
        assert np.array_equal(ref.words(), other.words())
    rec, dg = M.random_records(rng, n, 600, 3)
    perm = rng.sample(range(600), 600)
    assert ref.sent(X, rec, 600, dg) == other.sent(X, rec[perm].copy(), 600, dg[perm].copy())
    assert np.array_equal(ref.words(), other.words())
    pkts = [M.write_rr(Y.ssrc[s], [M.write_block(X.ssrc[(s + 1) % n], s, s, s, s, 1 + s, s)]) + M.write_sdes(Y.ssrc[s], b"q") for s in range(n)]
    pkts += [M.write_sr(Y.ssrc[s], s << 32, 0, 0, 0) for s in range(n)] + [M.write_rr(1, []) + M.write_bye([Y.ssrc[3]])]
    offs = np.cumsum([0] + [len(x) for x in pkts])
    wire = np.frombuffer(b"".join(pkts), np.uint8)
    dgr = np.array([(int(offs[k]), len(pkts[k])) for k in range(len(pkts))], np.int32)
    fa, ca = ref.parse(Y, X, dgr, wire, 1 << 40)
    fb, cb = other.parse(Y, X, dgr[rng.sample(range(len(pkts)), len(pkts))].copy(), wire, 1 << 40)
    assert ca == cb and np.array_equal(fa, fb) and np.array_equal(ref.words(), other.words()) and fa[3, 0] & M.BYE_BIT


def test_one_stream_owns_the_call(torch_cuda):
    """8192 datagrams of one stream among 8 (a flooding client), with losses and a wrap; then two flooding streams at once"""
    n = 8
    _, Y = sessions(n)
    impl, model = fresh(torch_cuda, n)
    rng = random.Random(2)
    items = [(2, q // 2, q & 1, 60000 + q + (q // 97), 1000 + q * 320 + rng.randrange(50)) for q in range(8192)]
    M.run_received(impl, model, Y, [M.make_tick(items, True, 0)], check)
    assert model.rows[2]["received"] > 8000 and model.rows[2]["cycles"] == 65536
    items = M.interleave(rng, [[(s, q, 0, 7 * s + q, 5 * q) for q in range(400 + 100 * s)] if s in (1, 6) else [(s, 0, 0, 1, 2)] for s in range(n)])
    M.run_received(impl, model, Y, [M.make_tick(items, False, 12345)], check)


def test_binding(torch_cuda):
    """solo_amd.Rtcp end to end: two sides exchange reports through build() and parse(); the checks of the arguments"""
    import solo_amd
    torch = torch_cuda
    n = 8
    X, Y = sessions(n)
    rx, ry = gpu_session(X), gpu_session(Y)
    a, b = solo_amd.Rtcp(n), solo_amd.Rtcp(n)
    model = M.Model(n)
    for o in (a, b):
        o.set_cname(range(n), ["s%d@example.net" % s for s in range(n)])
    model.set_cname(range(n), [b"s%d@example.net" % s for s in range(n)])
    tick = M.scenario("a", n, 1, 1, Y, [0] * n)[0]
    c = a.received(ry, dev(torch, tick["arrivals"]), dev(torch, tick["rtp_seq"].view(np.int16)), dev(torch, tick["arrival_time"].view(np.int32)))
    want = model.received(Y, tick["arrivals"], tick["rtp_seq"], tick["arrival_time"], 0)
    assert a.count("received", c) == want
    rec = np.array([(s, 4, 0, 0, 30) for s in range(n)], np.int32)
    dg = np.array([(0, 42)] * n, np.int32)
    c = a.sent(rx, dev(torch, rec), dev(torch, np.array([n] * 8, np.int32)), dev(torch, dg))
    assert a.count("sent", c) == model.sent(rec, n, dg)
    now = (0x83AA7E80 << 32) | 0x10000
    dgrams, wire, c = a.build(rx, ry, [1, 3, 4], now)
    _, md, mw, mc = model.build(X, Y, [1, 3, 4], now, 96 * 3)
    assert a.count("build", c) == mc and host(torch, dgrams).tolist() == [list(x) for x in md] and host(torch, wire)[:len(mw)].tobytes() == mw
    assert np.array_equal(np.ascontiguousarray(host(torch, a.get_state())).view(np.uint32), model.words())
    fb, c = b.parse(rx, ry, dgrams, wire, dev(torch, np.array([now + (7 << 16)], np.uint64).view(np.int64)))
    mb = M.Model(n)
    mfb, mc = mb.parse(X, Y, md, mw, now + (7 << 16))
    assert b.count("parse", c) == mc and mc["sr"] == 3 and mc["blocks"] == 3
    assert np.array_equal(host(torch, fb).view(np.uint32), M.feedback_array(mfb))
    a.reset([3])
    assert not np.ascontiguousarray(host(torch, a.get_state([3]))).any()
    for call in (lambda: a.received(rx, dgrams, wire), lambda: a.received(object(), dev(torch, tick["arrivals"]), dev(torch, tick["rtp_seq"].view(np.int16))),
                 lambda: a.sent(rx, dev(torch, rec), dev(torch, dg), dev(torch, dg)), lambda: a.build(rx, solo_amd.Rtp(n + 1), [0], 0),
                 lambda: a.build(rx, None, [2, 1], 0), lambda: a.build(rx, None, [0], -1), lambda: a.parse(rx, None, wire, wire, 0),
                 lambda: a.parse(rx, None, dgrams, wire, torch.zeros(2, dtype=torch.int64, device="cuda")), lambda: a.set_cname([0], ""),
                 lambda: a.set_cname([0, 0], "x"), lambda: a.count("nothing", c)):
        with pytest.raises(ValueError):
            call()
    a.close()
    b.close()


# ---- capture: the calls in linear graphs on one stream, replayed against eager twins and the model ------------------------------------------
def test_capture_received_tick(torch_cuda):
    """solo_rtp_parse, solo_rtcp_received and solo_recv_insert in one graph, a fixed capacity of 16 datagrams: replay k files packet k of
    the codec fixture with arrival times of its own; the statistics equal the twin's and the model's, and the ring plays the reference PCM"""
    import solo_amd
    import rtp_model as R
    import test_gpu_rtp as TR
    torch = torch_cuda
    z = G.fixture()
    pool, parts = G.datagrams()
    A, W, NP = 16, 8192, 4
    ses = TR._fixture_session()
    sm = M.Session([ses["streams"][s]["ssrc"] for s in range(8)], [ses["streams"][s]["ts_offset"] for s in range(8)], packet_samples=640)
    rng = np.random.default_rng(4)
    feeds = []
    for k in range(NP):
        dgs = []
        for (s, p, d), (off, ln) in sorted(parts.items()):
            if p == k:
                c = ses["streams"][s]
                dgs.append(R.build(c["ssrc"], c["pt"][d], 2 * k + d, c["ts_offset"] + k * 640, pool[off:off + ln].tobytes(), ext=R.level_ext(3, 16 * k + s)))
        dgs = [dgs[i] for i in rng.permutation(len(dgs))]
        table, wire = TR._lay_out(rng, dgs)
        dg = np.zeros((A, 2), np.int32)
        dg[:len(dgs)] = table
        w = np.zeros(W, np.uint8)
        w[:wire.size] = wire
        feeds.append(dict(dgrams=dg, wire=w, atime=rng.integers(-2 ** 31, 2 ** 31, A).astype(np.int32)))

    def make():
        h = solo_amd.SoloBatch(8, encoder=False, decoder=True, slot_bytes=512)
        h.recv_create(8, 256, 0)
        rtp = TR.gpu_session(ses)
        rtcp = solo_amd.Rtcp(8)
        ins = dict(dgrams=G.zeros(torch, (A, 2), torch.int32), wire=G.zeros(torch, (W,), torch.uint8), atime=G.zeros(torch, (A,), torch.int32))
        outs = dict(arrivals=G.zeros(torch, (A, 5), torch.int32), rtp_seq=G.zeros(torch, (A,), torch.int16), count=G.zeros(torch, (8,), torch.int32),
                    rcount=G.zeros(torch, (8,), torch.int32))

        def call():
            r = rtp.lib.solo_rtp_parse(rtp.h, h.h, ins["dgrams"].data_ptr(), A, ins["wire"].data_ptr(), W, outs["arrivals"].data_ptr(), None,
                                       outs["rtp_seq"].data_ptr(), outs["count"].data_ptr(), rtp._stream())
            r = r or rtcp.lib.solo_rtcp_received(rtcp.h, rtp.h, outs["arrivals"].data_ptr(), outs["rtp_seq"].data_ptr(), A, ins["atime"].data_ptr(), 0,
                                                 outs["rcount"].data_ptr(), rtcp._stream())
            return r or h.lib.solo_recv_insert(h.h, outs["arrivals"].data_ptr(), A, ins["wire"].data_ptr(), W, h._stream())

        def state():
            s = h.recv_stats()
            return np.concatenate([np.array([s[f] for f in ("inserted", "late", "ahead", "duplicate", "bad")], np.int64),
                                   np.ascontiguousarray(host(torch, rtcp.get_state())).view(np.uint32).ravel().astype(np.int64)])
        return G.Stage(torch, ins, outs, call, state=state, keep=(h, rtp, rtcp))

    mdl = M.Model(8)

    def model(k, feed, got):
        want = mdl.received(sm, got["arrivals"], got["rtp_seq"].view(np.uint16), feed["atime"].view(np.uint32), 0)
        assert want["counted"] > 0 and got["rcount"][:7].tolist() == [want[f] for f in M.RECEIVED_COUNT], (k, want, got["rcount"])

    _, cap, twin = G.replay_against_twin(torch, make, feeds, model=model, stateful=True)
    assert np.array_equal(cap.state()[5:].astype(np.uint32).reshape(8, 40), mdl.words())
    assert any(r["jitter"] for r in mdl.rows)
    for st in (cap, twin):
        pcm, status = st.keep[0].recv_decode(NP)
        assert int(host(torch, status).max()) == 0
        assert np.array_equal(host(torch, pcm), z["dec_loss"][:, :NP])


def test_capture_sent_tick(torch_cuda):
    """solo_send_pack, solo_rtp_pack and solo_rtcp_sent behind them in one graph: the record count travels on the device"""
    import solo_amd
    import test_gpu_rtp as TR
    torch = torch_cuda
    z = G.fixture()
    P, SLOT, MAXR, WCAP = 3, z["bits"].shape[2], 48, 16384
    ses = TR._fixture_session()

    def make():
        h = solo_amd.SoloBatch(8, encoder=False, decoder=True, slot_bytes=SLOT)
        rtp = TR.gpu_session(ses)
        rtcp = solo_amd.Rtcp(8)
        ins = dict(bits=G.zeros(torch, (8, P, SLOT), torch.uint8), nbytes=G.zeros(torch, (8, P, 2), torch.int16))
        outs = dict(records=G.zeros(torch, (MAXR, 5), torch.int32), payload=G.zeros(torch, (8 * P * SLOT,), torch.uint8), scount=G.zeros(torch, (8,), torch.int32),
                    dgrams=G.zeros(torch, (MAXR, 2), torch.int32), wire=G.zeros(torch, (WCAP,), torch.uint8), count=G.zeros(torch, (8,), torch.int32),
                    tcount=G.zeros(torch, (8,), torch.int32))

        def call():
            r = h.lib.solo_send_pack(h.h, ins["bits"].data_ptr(), ins["nbytes"].data_ptr(), None, P, None, 500, outs["records"].data_ptr(), MAXR,
                                     outs["payload"].data_ptr(), 8 * P * SLOT, outs["scount"].data_ptr(), h._stream())
            r = r or rtp.lib.solo_rtp_pack(rtp.h, outs["records"].data_ptr(), outs["scount"].data_ptr(), MAXR, outs["payload"].data_ptr(), 8 * P * SLOT,
                                           None, 0, outs["dgrams"].data_ptr(), outs["wire"].data_ptr(), WCAP, outs["count"].data_ptr(), rtp._stream())
            return r or rtcp.lib.solo_rtcp_sent(rtcp.h, rtp.h, outs["records"].data_ptr(), outs["scount"].data_ptr(), MAXR, outs["dgrams"].data_ptr(),
                                                outs["tcount"].data_ptr(), rtcp._stream())

        def state():
            return np.ascontiguousarray(host(torch, rtcp.get_state())).view(np.uint32)
        return G.Stage(torch, ins, outs, call, state=state, keep=(h, rtp, rtcp))

    feeds = [dict(bits=z["bits"][:, 3 * k:3 * k + 3], nbytes=z["nbytes"][:, 3 * k:3 * k + 3]) for k in range(4)]
    mdl = M.Model(8)

    def model(k, feed, got):
        n = int(got["scount"][0])
        want = mdl.sent(got["records"], n, got["dgrams"])
        assert 0 < n <= MAXR and want["sent"] == n and got["tcount"][:2].tolist() == [want["sent"], want["skipped"]], (k, n, want, got["tcount"])

    _, cap, twin = G.replay_against_twin(torch, make, feeds, model=model, stateful=True)
    assert np.array_equal(cap.state(), mdl.words()) and all(r["tx_next"] == 503 and r["tx_since"] > 0 for r in mdl.rows)


def test_capture_build_and_parse(torch_cuda):
    """solo_rtcp_build of side A and solo_rtcp_parse of side B behind it in one graph, the time taken from a device word: every replay
    stamps another time, and between the replays A goes on sending and receiving eagerly"""
    import solo_amd
    torch = torch_cuda
    n, CAP = 70, 96 * 70
    X, Y = sessions(n)
    rx, ry = gpu_session(X), gpu_session(Y)
    names = [b"s%d@example.net" % s for s in range(n)]
    ticks = M.scenario("b", n, 5, 31, Y, [100] * n)
    rec = np.array([(s, 10, 0, 0, 33 + s) for s in range(0, n, 2)], np.int32)
    dg = np.array([(0, 45)] * len(rec), np.int32)
    streams = list(range(1, n))

    def make():
        a, b = GpuRtcp(torch, n), GpuRtcp(torch, n)
        assert a.set_cname(list(range(n)), names) == 0
        ins = dict(now=G.zeros(torch, (1,), torch.int64))
        outs = dict(dgrams=G.zeros(torch, (n - 1, 2), torch.int32), wire=G.zeros(torch, (CAP,), torch.uint8), count=G.zeros(torch, (8,), torch.int32),
                    feedback=G.zeros(torch, (n, 8), torch.int32), pcount=G.zeros(torch, (16,), torch.int32))
        idx = dev(torch, np.array(streams, np.int32))

        def call():
            r = a.lib.solo_rtcp_build(a.h, rx.h, ry.h, idx.data_ptr(), n - 1, 1, ins["now"].data_ptr(), outs["dgrams"].data_ptr(), outs["wire"].data_ptr(), CAP,
                                      outs["count"].data_ptr(), a.o._stream())
            return r or b.lib.solo_rtcp_parse(b.h, rx.h, ry.h, outs["dgrams"].data_ptr(), n - 1, outs["wire"].data_ptr(), CAP, 2, ins["now"].data_ptr(),
                                              outs["feedback"].data_ptr(), outs["pcount"].data_ptr(), b.o._stream())

        def state():
            return np.concatenate([a.words(), b.words()])
        return G.Stage(torch, ins, outs, call, state=state, keep=(a, b, idx))

    def between(stage, k):
        a = stage.keep[0]
        a.received(Y, ticks[k])
        a.sent(X, rec, len(rec) if k % 2 == 0 else 3, dg)

    ma, mb = M.Model(n), M.Model(n)
    ma.set_cname(list(range(n)), names)
    feeds = [dict(now=np.array([(0x83AA7E80 + 5 * k << 32) | (k << 20)], np.uint64).view(np.int64)) for k in range(5)]

    def model(k, feed, got):
        now = int(feed["now"].view(np.uint64)[0])
        ma.received(Y, ticks[k]["arrivals"], ticks[k]["rtp_seq"], ticks[k]["arrival_time"], ticks[k]["now_rtp"])
        ma.sent(rec, len(rec) if k % 2 == 0 else 3, dg)
        _, md, mw, mc = ma.build(X, Y, streams, now, CAP)
        mfb, pc = mb.parse(X, Y, md, mw, now)
        assert build_count_of(got["count"]) == mc and mc["with_sr"] > 0 and got["dgrams"].tolist() == [list(x) for x in md], (k, mc)
        assert got["wire"][:len(mw)].tobytes() == mw and (got["wire"][len(mw):] == G.FILL).all()
        assert got["pcount"][:10].tolist() == [pc[f] for f in M.PARSE_COUNT] and pc["blocks"] > 0
        assert np.array_equal(got["feedback"].view(np.uint32), M.feedback_array(mfb))

    _, cap, twin = G.replay_against_twin(torch, make, feeds, model=model, between=between, stateful=True)
    assert np.array_equal(cap.state(), np.concatenate([ma.words(), mb.words()]))

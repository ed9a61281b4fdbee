"""SRTCP on the GPU (solo_srtcp_protect / solo_srtcp_unprotect and solo_rtcp_set_trailer through the C ABI, the keys through solo_amd.Rtp)
against the independent model of tests/srtcp_model.py, byte for byte: protect over 1 and 257 listed streams (one full tile of 256
datagrams plus one) with the families of tests/test_srtcp_model.py, unprotect over 1 and 257 datagrams with the hostile set at all four
byte alignments, the secured loop against the loop in the clear at 70 streams, the control plane on the device, and both device calls
captured in graphs and replayed against eager twins.

CAPTURED names the test that captures each of the two calls the interface calls capturable (tests/test_srtcp_model.py holds this file
and the header to it)."""
import copy
import ctypes as C

import numpy as np
import pytest

import graph_replay_lib as G
import rtcp_model as R
import srtcp_model as M
import test_srtcp_model as CPU

pytestmark = pytest.mark.gpu
CAPTURED = {"solo_srtcp_protect": "test_capture_rtcp_build_and_srtcp_protect", "solo_srtcp_unprotect": "test_capture_srtcp_unprotect_and_rtcp_parse"}
FILL8, FILL32 = 0xA5, -7
NOW = CPU.NOW
ZERO = dict.fromkeys(M.VERDICTS, 0)


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


def count_dict(cnt):
    return dict(zip(M.VERDICTS, (int(v) for v in cnt)))


def gpu_session(ses, keys=None, tx_state=None, rx_state=None):
    """a solo_amd.Rtp bound as the model's Session says and keyed for SRTCP through the binding"""
    import solo_amd
    r = solo_amd.Rtp(ses.n, ses.L)
    s = [k for k in range(ses.n) if ses.bound[k]]
    r.bind(s, [ses.ssrc[k] for k in s], [ses.ts_offset[k] for k in s], 0, (96, 97), 0)
    for d in ("tx", "rx"):
        ss = sorted(k for k, v in (keys or {}).items() if v.get(d) is not None)
        if ss and d == "tx":
            r.set_rtcp_keys(ss, tx=[keys[k]["tx"] for k in ss], tx_index=[(tx_state or {}).get(k, 0) for k in ss])
        elif ss:
            r.set_rtcp_keys(ss, rx=[keys[k]["rx"] for k in ss], rx_index=[(rx_state or {}).get(k, -1) for k in ss])
    return r


class GpuRtcp:
    """a solo_rtcp_t with the trailer switch, driven through the C ABI with guarded buffers"""

    def __init__(self, torch, n, words=None, trailer=None):
        import solo_amd
        self.torch, self.n = torch, n
        self.o = solo_amd.Rtcp(n)
        self.lib, self.h = self.o.lib, self.o.h
        if words is not None:
            self.set_words(words)
        if trailer is not None:
            self.o.set_trailer(trailer)

    def words(self):
        return np.ascontiguousarray(host(self.torch, self.o.get_state())).view(np.uint32)

    def set_words(self, w):
        self.o.set_state(dev(self.torch, np.ascontiguousarray(w, np.uint32).view(np.uint8).reshape(self.n, 160)))

    def build(self, tx, rx, streams, now, cap, room, guard=64):
        """-> (dgrams, wire, count: device tensors with guards behind n / room / 8, the list on the device)"""
        t = self.torch
        idx = dev(t, np.asarray(streams, np.int32))
        dg = t.full((len(streams) + 2, 2), FILL32, dtype=t.int32, device="cuda")
        wire = t.full((room + guard,), FILL8, dtype=t.uint8, device="cuda")
        cnt = t.full((12,), FILL32, dtype=t.int32, device="cuda")
        r = self.lib.solo_rtcp_build(self.h, tx.h, None if rx is None else rx.h, idx.data_ptr(), len(streams), now, None, dg.data_ptr(), wire.data_ptr(), cap,
                                     cnt.data_ptr(), self.o._stream())
        assert r == 0
        return dg, wire, cnt, idx


def protect(torch, rtcp, ses, idx, bcnt, dg, wire, wire_bytes):
    cnt = torch.full((12,), -9, dtype=torch.int32, device="cuda")
    r = ses.lib.solo_srtcp_protect(rtcp.h, ses.h, idx.data_ptr(), int(idx.shape[0]), bcnt.data_ptr(), dg.data_ptr(), wire.data_ptr(), wire_bytes, cnt.data_ptr(),
                                   ses._stream())
    assert r == 0
    cnt = host(torch, cnt)
    assert (cnt[8:] == -9).all()
    return count_dict(cnt[:8])


def unprotect(torch, ses, dg, wire, out=None):
    n = int(dg.shape[0])
    out = torch.full((n + 4, 2), FILL32, dtype=torch.int32, device="cuda") if out is None else out
    cnt = torch.full((12,), -9, dtype=torch.int32, device="cuda")
    r = ses.lib.solo_srtcp_unprotect(ses.h, dg.data_ptr(), n, wire.data_ptr(), int(wire.shape[0]), out.data_ptr(), cnt.data_ptr(), ses._stream())
    assert r == 0
    cnt = host(torch, cnt)
    assert (cnt[8:] == -9).all()
    return out, count_dict(cnt[:8])


# ---- protect ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 257])
def test_protect_against_the_model(torch_cuda, n):
    torch = torch_cuda
    N = 12 if n == 1 else 260
    rng = np.random.default_rng(100 + n)
    X, Y = CPU.sessions(N)
    X.bound[9] = 0
    keys = M.random_keys(rng, range(N), no_tx=(5,))
    tx_state = {s: CPU.PROTECT_INDEX.get(s, int(rng.integers(0, 2 ** 31 - 10))) for s in range(N)}
    tx_state[5] = 0                                                   # (no tx key: no send index either)
    model = CPU.fill_state(rng, R.Model(N), CPU.PROTECT_SHAPES)
    g = GpuRtcp(torch, N, model.words(), trailer=14)
    tx, rx = gpu_session(X, keys, tx_state), gpu_session(Y)
    streams = [1] if n == 1 else list(range(n))
    for call in range(2):
        need = M.model_build_trailer(copy.deepcopy(model), X, Y, streams, NOW + call, 2 ** 40, 14)[3]["bytes_needed"]
        cap = need - 1 if call == 0 and n > 1 else need               # the first call's cap cuts the last listed packet
        dg, wire, bcnt, idx = g.build(tx, rx, streams, NOW + call, cap, need)
        refused, mdg, mwire, mc = M.model_build_trailer(model, X, Y, streams, NOW + call, cap, 14)
        hdg, hwire, hb = host(torch, dg), host(torch, wire), host(torch, bcnt)
        assert CPU.build_count_of(hb[:8]) == mc and hdg[:len(streams)].tolist() == [list(d) for d in mdg] and (hdg[len(streams):] == FILL32).all()
        assert hwire[:len(mwire)].tobytes() == mwire and (hwire[len(mwire):] == FILL8).all() and np.array_equal(g.words(), model.words())
        want = M.model_protect(keys, tx_state, N, streams, False, hdg[:len(streams)], hwire)
        got = protect(torch, g.o, tx, idx, bcnt, dg, wire, int(wire.shape[0]))
        assert got == want["count"], (got, want["count"])
        hdg, hwire = host(torch, dg), host(torch, wire)
        assert np.array_equal(hdg[:len(streams)], want["dgrams"]) and (hdg[len(streams):] == FILL32).all()         # guards hold behind the list ...
        assert np.array_equal(hwire, want["wire"]) and (hwire[need:] == FILL8).all()                                   # ... and behind the wire
        tx_state = want["tx_state"]
        assert tx.rtcp_index() == ([tx_state[s] for s in range(N)], [-1] * N)
        if n > 1:
            assert got["no_key"] == 1 and got["exhausted"] == 1 + call and got["skipped"] == 2 - call and got["ok"] == n - 4
    if n == 1:
        return
    # a refused list: ok = -1, nothing touched
    dg, wire, bcnt, idx = g.build(tx, rx, [3, 2], NOW, 2 ** 40, 224)
    assert host(torch, bcnt)[0] == -1
    dg[:2] = dev(torch, np.array([[0, 48], [48, 48]], np.int32))
    keep_dg, keep_wire = host(torch, dg).copy(), host(torch, wire).copy()
    assert protect(torch, g.o, tx, idx, bcnt, dg, wire, int(wire.shape[0])) == dict(ZERO, ok=-1)
    assert np.array_equal(host(torch, dg), keep_dg) and np.array_equal(host(torch, wire), keep_wire) and tx.rtcp_index()[0] == [tx_state[s] for s in range(N)]
    # each -1 of the C ABI: nothing is enqueued
    ok = torch.zeros((8,), dtype=torch.int32, device="cuda")
    cnt = torch.full((8,), -9, dtype=torch.int32, device="cuda")
    g13, g9, r9 = GpuRtcp(torch, N, trailer=13), GpuRtcp(torch, N + 1, trailer=14), gpu_session(R.Session([1, 2], [0, 0]))
    a = dict(c=g.h, r=tx.h, streams=idx.data_ptr(), n=2, bc=ok.data_ptr(), dg=dg.data_ptr(), wire=wire.data_ptr(), wb=200, cnt=cnt.data_ptr())
    for over in (dict(c=None), dict(r=None), dict(streams=None), dict(bc=None), dict(dg=None), dict(wire=None), dict(cnt=None), dict(n=0), dict(n=N + 1), dict(wb=-1),
                 dict(c=g13.h), dict(c=g9.h), dict(r=r9.h), dict(streams=idx.data_ptr() + 2), dict(dg=dg.data_ptr() + 2), dict(wire=wire.data_ptr() + 1),
                 dict(cnt=cnt.data_ptr() + 2), dict(bc=ok.data_ptr() + 4)):
        b = dict(a, **over)
        assert tx.lib.solo_srtcp_protect(b["c"], b["r"], b["streams"], b["n"], b["bc"], b["dg"], b["wire"], b["wb"], b["cnt"], tx._stream()) == -1, over
    assert (host(torch, cnt) == -9).all() and np.array_equal(host(torch, wire), keep_wire)
    assert g.lib.solo_rtcp_set_trailer(None, 14) == -1 and g.lib.solo_rtcp_set_trailer(g.h, 17) == -1 and g.lib.solo_rtcp_set_trailer(g.h, -1) == -1


# ---- unprotect -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 257])
def test_unprotect_against_the_model(torch_cuda, n):
    torch = torch_cuda
    rng = np.random.default_rng(200 + n)
    Y, keys, rx_state, items = CPU.receive_case(rng)
    if n == 1:
        packets, align = [items[[k[0] for k in items].index("large")][1]], [3]
    else:
        packets = [k[1] for k in items] * 4                            # the hostile set at all four alignments (a copy of an accepted datagram passes too)
        align = [a for a in range(4) for _ in items]
        k11 = M.session_keys(keys[11]["rx"])
        extra = n - 3 - len(packets)
        packets += [M.protect_packet(k11, R.write_rr(Y.ssrc[11]) + R.write_sdes(Y.ssrc[11], b"n" * (1 + i % 31)), 100 + i) for i in range(extra)]
        align += [i % 4 for i in range(extra)]
    dg, wire = M.lay_out(rng, packets, align=align)
    if n > 1:
        assert sorted(set(int(o) % 4 for o in dg[:len(items) * 4, 0])) == [0, 1, 2, 3]
        dg = np.concatenate([dg, np.array([[wire.size - 10, 40], [-4, 30], [wire.size, 22]], np.int32)])
    assert dg.shape[0] == n
    want = M.model_unprotect(Y, keys, rx_state, dg, wire)
    if n > 1:
        assert want["verdicts"][:len(items)] == [k[2] for k in items] and all(want["count"][v] > 0 for v in M.VERDICTS[2:7])
    ses = gpu_session(Y, keys, rx_state=rx_state)
    ddg, dw = dev(torch, dg), dev(torch, wire)
    out, cnt = unprotect(torch, ses, ddg, dw)
    hout, hw = host(torch, out), host(torch, dw)
    assert cnt == want["count"], (cnt, want["count"])
    assert np.array_equal(hout[:n], want["dgrams"]) and (hout[n:] == FILL32).all() and np.array_equal(hw, want["wire"])
    assert ses.rtcp_index()[1] == [want["rx_state"][s] for s in range(Y.n)]
    # the same datagrams again, into the list itself: what was accepted is now replayed, every byte kept
    again = M.model_unprotect(Y, keys, want["rx_state"], dg, hw)
    out2, cnt2 = unprotect(torch, ses, ddg, dw, out=ddg)
    assert cnt2 == again["count"] and cnt2["ok"] == 0 and cnt2["replayed"] >= want["count"]["ok"] > 0
    assert np.array_equal(host(torch, dw), hw) and not host(torch, ddg).any() and ses.rtcp_index()[1] == [want["rx_state"][s] for s in range(Y.n)]
    if n == 1:
        return
    cnt = torch.full((8,), -9, dtype=torch.int32, device="cuda")
    a = dict(r=ses.h, dg=ddg.data_ptr(), n=4, wire=dw.data_ptr(), wb=100, out=out.data_ptr(), cnt=cnt.data_ptr())
    for over in (dict(r=None), dict(cnt=None), dict(n=-1), dict(wb=-1), dict(dg=None), dict(wire=None), dict(out=None), dict(dg=ddg.data_ptr() + 2),
                 dict(out=out.data_ptr() + 1), dict(cnt=cnt.data_ptr() + 2)):
        b = dict(a, **over)
        assert ses.lib.solo_srtcp_unprotect(b["r"], b["dg"], b["n"], b["wire"], b["wb"], b["out"], b["cnt"], ses._stream()) == -1, over
    assert (host(torch, cnt) == -9).all()
    assert ses.lib.solo_srtcp_unprotect(ses.h, None, 0, None, 0, None, cnt.data_ptr(), ses._stream()) == 0 and count_dict(host(torch, cnt)) == ZERO


# ---- the loop ----------------------------------------------------------------------------------------------------------------------------------
def test_secured_loop_equals_the_loop_in_the_clear(torch_cuda):
    """rtcp_build -> srtcp_protect -> (copy) -> srtcp_unprotect -> rtcp_parse gives d_feedback, both count records and the whole RTCP state
    bit for bit as the same chain in the clear, and no cleartext body byte survives on the wire"""
    torch = torch_cuda
    n = 70
    rng = np.random.default_rng(300)
    X, Y = CPU.sessions(n)
    keys = M.random_keys(rng, range(n))
    wa, wb = CPU.fill_state(rng, R.Model(n)).words(), CPU.fill_state(rng, R.Model(n)).words()
    A, B = GpuRtcp(torch, n, wa, trailer=14), GpuRtcp(torch, n, wb)
    A2, B2 = GpuRtcp(torch, n, wa), GpuRtcp(torch, n, wb)
    tx, ry = gpu_session(X, keys), gpu_session(Y)
    peer, ours = gpu_session(X, M.loop_keys(keys)), gpu_session(Y)             # the receiving side: the peers' SSRCs with their keys, and its own
    streams = list(range(n))
    for tick in range(2):
        now = NOW + (tick << 32)
        dg, wire, bcnt, idx = A.build(tx, ry, streams, now, 2 ** 40, 112 * n)
        dgp, wirep, bcntp, _ = A2.build(tx, ry, streams, now, 2 ** 40, 112 * n)
        pc = protect(torch, A.o, tx, idx, bcnt, dg, wire, int(wire.shape[0]))
        assert pc == dict(ZERO, ok=n)
        hdg, hw, hdgp, hwp = host(torch, dg)[:n], host(torch, wire), host(torch, dgp)[:n], host(torch, wirep)
        b1, b2 = CPU.build_count_of(host(torch, bcnt)[:8]), CPU.build_count_of(host(torch, bcntp)[:8])
        assert b1 == dict(b2, bytes=b2["bytes"] + 16 * n, bytes_needed=b2["bytes_needed"] + 16 * n) and b1["built"] == n
        for (off, ln), (po, pl) in zip(hdg.tolist(), hdgp.tolist()):
            assert ln == pl + 14 and np.array_equal(hw[off:off + 8], hwp[po:po + 8])
            assert pl <= 8 or not np.array_equal(hw[off + 8:off + pl], hwp[po + 8:po + pl])
        moved = torch.zeros((int(wire.shape[0]) + 3,), dtype=torch.uint8, device="cuda")         # the copy: the receiver's buffer, at another alignment
        moved[3:] = wire
        dgr = dev(torch, hdg + np.array([3, 0], np.int32))
        out, uc = unprotect(torch, peer, dgr, moved)
        assert uc == dict(ZERO, ok=n)
        fb, pcnt = B.o.parse(peer, ours, out[:n].contiguous(), moved, now + 5)
        fb2, pcnt2 = B2.o.parse(peer, ours, dgp[:n].contiguous(), wirep, now + 5)
        assert np.array_equal(host(torch, fb), host(torch, fb2)) and np.array_equal(host(torch, pcnt), host(torch, pcnt2)) and host(torch, pcnt)[0] == n
        assert np.array_equal(A.words(), A2.words()) and np.array_equal(B.words(), B2.words())
        assert tx.rtcp_index()[0] == [tick + 1] * n and peer.rtcp_index()[1] == [tick] * n


# ---- the control plane on the device -------------------------------------------------------------------------------------------------------------
def test_control_plane(torch_cuda):
    """SRTP keys alone leave the SRTCP allocation absent; solo_srtp_clear_keys does not touch SRTCP; clear_rtcp_keys and unbind wipe;
    rtcp_index and set_rtcp_keys hand a stream over to another session"""
    torch = torch_cuda
    n = 6
    rng = np.random.default_rng(400)
    _, Y = CPU.sessions(n)
    keys = M.random_keys(rng, range(n))
    ses = gpu_session(Y)
    d = [M.protect_packet(M.session_keys(keys[s]["rx"]), R.write_rr(Y.ssrc[s]) + R.write_sdes(Y.ssrc[s], b"cp"), 7) for s in range(n)]
    dg, wire = M.lay_out(rng, d)
    ddg = dev(torch, dg)

    def verdicts():
        out, cnt = unprotect(torch, ses, ddg, dev(torch, wire))
        return cnt
    ses.set_trailer(10)
    ses.set_keys([0, 1], tx=[keys[0]["tx"], keys[1]["tx"]], rx=[keys[0]["rx"], keys[1]["rx"]])
    assert ses.rtcp_index() == ([0] * n, [-1] * n) and verdicts() == dict(ZERO, no_key=n)          # SRTP keys are no SRTCP keys
    ses.set_rtcp_keys([0, 1, 2], rx=[keys[s]["rx"] for s in (0, 1, 2)], rx_index=[-1, 6, 7])
    ses.set_rtcp_keys([1], tx=[keys[1]["tx"]], tx_index=2 ** 31)
    assert ses.rtcp_index() == ([0, 2 ** 31, 0, 0, 0, 0], [-1, 6, 7, -1, -1, -1])
    ses.clear_keys([0, 1, 2])                                                                     # SRTP's clear: SRTCP stays
    assert ses.rtcp_index([1, 2]) == ([2 ** 31, 0], [6, 7]) and verdicts() == dict(ZERO, ok=2, replayed=1, no_key=3)
    assert ses.rtcp_index()[1] == [7, 7, 7, -1, -1, -1]
    for kw in (dict(tx_index=[2 ** 31 + 1]), dict(rx_index=[2 ** 31])):                            # the C ABI's own refusals: nothing changes
        ti = None if "tx_index" not in kw else (C.c_uint32 * 1)(*kw["tx_index"])
        ri = None if "rx_index" not in kw else (C.c_int64 * 1)(*kw["rx_index"])
        assert ses.lib.solo_srtcp_set_keys(ses.h, (C.c_int32 * 1)(1), 1, keys[3]["tx"], keys[3]["rx"], ti, ri, ses._stream()) == -1
    assert ses.lib.solo_srtcp_set_keys(ses.h, (C.c_int32 * 1)(1), 1, None, None, None, None, ses._stream()) == -1
    assert ses.lib.solo_srtcp_set_keys(ses.h, (C.c_int32 * 2)(1, 1), 2, keys[3]["tx"] * 2, None, None, None, ses._stream()) == -1
    assert ses.rtcp_index() == ([0, 2 ** 31, 0, 0, 0, 0], [7, 7, 7, -1, -1, -1])
    # the hand-over: another session takes the records and rejects what the first one has seen
    other = gpu_session(Y)
    txn, rxi = ses.rtcp_index([0, 1, 2])
    other.set_rtcp_keys([0, 1, 2], tx=[keys[s]["tx"] for s in (0, 1, 2)], rx=[keys[s]["rx"] for s in (0, 1, 2)], tx_index=txn, rx_index=rxi)
    assert other.rtcp_index([0, 1, 2]) == (txn, rxi)
    out, cnt = unprotect(torch, other, ddg, dev(torch, wire))
    assert cnt == dict(ZERO, replayed=3, no_key=3)
    ses.clear_rtcp_keys([1])
    ses.unbind([2])
    assert ses.rtcp_index() == ([0] * n, [7, -1, -1, -1, -1, -1]) and verdicts() == dict(ZERO, replayed=1, no_key=4, unknown_ssrc=1)


# ---- capture -------------------------------------------------------------------------------------------------------------------------------------
def test_capture_rtcp_build_and_srtcp_protect(torch_cuda):
    """solo_rtcp_build with the trailer and solo_srtcp_protect behind it in one graph: every replay stamps another time and ADVANCES THE
    SEND INDICES, so its bytes differ from the replay before and equal the model's"""
    torch = torch_cuda
    n, CAP = 70, 112 * 70
    rng = np.random.default_rng(500)
    X, Y = CPU.sessions(n)
    keys = M.random_keys(rng, range(n), no_tx=(5,))
    start = {s: int(rng.integers(0, 70000)) for s in range(n)}
    model = CPU.fill_state(rng, R.Model(n))
    w0 = model.words().copy()
    ry = gpu_session(Y)
    streams = list(range(1, n))

    def make():
        a, tx = GpuRtcp(torch, n, w0, trailer=14), gpu_session(X, keys, start)
        ins = dict(now=G.zeros(torch, (1,), torch.int64))
        outs = dict(dgrams=G.zeros(torch, (n - 1, 2), torch.int32), wire=G.zeros(torch, (CAP,), torch.uint8), bcount=G.zeros(torch, (8,), torch.int32),
                    count=G.zeros(torch, (8,), torch.int32))
        idx = dev(torch, np.array(streams, np.int32))

        def call():
            r = a.lib.solo_rtcp_build(a.h, tx.h, ry.h, idx.data_ptr(), n - 1, 1, ins["now"].data_ptr(), outs["dgrams"].data_ptr(), outs["wire"].data_ptr(), CAP,
                                      outs["bcount"].data_ptr(), a.o._stream())
            return r or tx.lib.solo_srtcp_protect(a.h, tx.h, idx.data_ptr(), n - 1, outs["bcount"].data_ptr(), outs["dgrams"].data_ptr(), outs["wire"].data_ptr(), CAP,
                                                  outs["count"].data_ptr(), tx._stream())

        def state():
            return np.concatenate([a.words().ravel(), np.array(tx.rtcp_index()[0], np.uint32)])
        return G.Stage(torch, ins, outs, call, state=state, keep=(a, tx, idx))

    feeds = [dict(now=np.array([(0x83AA7E80 + 5 * k << 32) | (k << 20)], np.uint64).view(np.int64)) for k in range(3)]
    tx_state = dict(start)

    def check(k, feed, got):
        nonlocal tx_state
        now = int(feed["now"].view(np.uint64)[0])
        _, md, mw, mc = M.model_build_trailer(model, X, Y, streams, now, CAP, 14)
        plain = np.full(CAP, G.FILL, np.uint8)
        plain[:len(mw)] = np.frombuffer(mw, np.uint8)
        want = M.model_protect(keys, tx_state, n, streams, False, md, plain)
        assert CPU.build_count_of(got["bcount"]) == mc and count_dict(got["count"]) == want["count"] == dict(ZERO, ok=n - 2, no_key=1)
        assert np.array_equal(got["dgrams"], want["dgrams"]) and np.array_equal(got["wire"], want["wire"])
        tx_state = want["tx_state"]

    _, cap, twin = G.replay_against_twin(torch, make, feeds, model=check, stateful=True)
    index = cap.keep[1].rtcp_index()[0]
    assert all(index[s] == tx_state[s] == start[s] + 3 for s in streams if s != 5) and index[0] == start[0] and index[5] == 0


def test_capture_srtcp_unprotect_and_rtcp_parse(torch_cuda):
    """solo_srtcp_unprotect and solo_rtcp_parse behind it in one graph, the received bytes copied into the working buffer by the graph
    itself: every replay brings datagrams with newer indices, one of them a replay of the call before"""
    torch = torch_cuda
    n = 70
    rng = np.random.default_rng(600)
    X, Y = CPU.sessions(n)
    keys = M.random_keys(rng, range(n), no_rx=(9,))
    sender = CPU.fill_state(rng, R.Model(n))
    feeds = []
    for k in range(3):
        now = NOW + (k << 32)
        for r in sender.rows:
            r["tx_since"] = 1 + k
        _, md, mw, _ = M.model_build_trailer(sender, X, Y, list(range(n)), now, 2 ** 40, 14)
        # the peers send with the keys this side receives with; stream 3 never moves on from index 0: from the second call on a replay
        want = M.model_protect({s: dict(tx=v["rx"]) for s, v in keys.items()}, {s: k if s != 3 else 0 for s in range(n)}, n, list(range(n)), False, md,
                               np.frombuffer(mw, np.uint8))
        dg = want["dgrams"].copy()
        dg[9] = md[9]                                                  # the stream without a key: its packet arrives as it is
        dg[9, 1] += 14
        wire = np.zeros(112 * n + 3, np.uint8)
        wire[3:3 + want["wire"].size] = want["wire"]
        feeds.append(dict(dgrams=dg + np.array([3, 0], np.int32), wire=wire, now=np.array([now + 9], np.uint64).view(np.int64)))
    ours = gpu_session(Y)
    w0 = CPU.fill_state(rng, R.Model(n)).words()

    def make():
        b, ses = GpuRtcp(torch, n, w0), gpu_session(X, keys)
        ins = dict(dgrams=G.zeros(torch, (n, 2), torch.int32), wire=G.zeros(torch, (112 * n + 3,), torch.uint8), now=G.zeros(torch, (1,), torch.int64))
        outs = dict(work=G.zeros(torch, (112 * n + 3,), torch.uint8), out=G.zeros(torch, (n, 2), torch.int32), count=G.zeros(torch, (8,), torch.int32),
                    feedback=G.zeros(torch, (n, 8), torch.int32), pcount=G.zeros(torch, (16,), torch.int32))

        def call():
            outs["work"].copy_(ins["wire"])
            r = ses.lib.solo_srtcp_unprotect(ses.h, ins["dgrams"].data_ptr(), n, outs["work"].data_ptr(), 112 * n + 3, outs["out"].data_ptr(), outs["count"].data_ptr(),
                                             ses._stream())
            return r or b.lib.solo_rtcp_parse(b.h, ses.h, ours.h, outs["out"].data_ptr(), n, outs["work"].data_ptr(), 112 * n + 3, 2, ins["now"].data_ptr(),
                                              outs["feedback"].data_ptr(), outs["pcount"].data_ptr(), b.o._stream())

        def state():
            return np.concatenate([b.words().ravel().astype(np.int64), np.array(ses.rtcp_index()[1], np.int64)])
        return G.Stage(torch, ins, outs, call, state=state, keep=(b, ses))

    mb = R.Model(n)
    mb.set_words(w0)
    rx_state = {s: -1 for s in range(n)}

    def check(k, feed, got):
        nonlocal rx_state
        want = M.model_unprotect(X, keys, rx_state, feed["dgrams"], feed["wire"])
        assert count_dict(got["count"]) == want["count"] == dict(ZERO, ok=n - 1 - (k > 0), no_key=1, replayed=int(k > 0))
        assert np.array_equal(got["out"], want["dgrams"]) and np.array_equal(got["work"], want["wire"])
        rx_state = want["rx_state"]
        mfb, pc = mb.parse(X, Y, want["dgrams"], want["wire"], int(feed["now"].view(np.uint64)[0]))
        assert got["pcount"][:10].tolist() == [pc[f] for f in R.PARSE_COUNT] and pc["accepted"] == n - 1 - (k > 0) and pc["malformed"] == 1 + (k > 0)
        assert np.array_equal(got["feedback"].view(np.uint32), R.feedback_array(mfb))

    _, cap, twin = G.replay_against_twin(torch, make, feeds, model=check, stateful=True)
    assert cap.keep[1].rtcp_index()[1] == [rx_state[s] for s in range(n)] and np.array_equal(cap.keep[0].words(), mb.words())

"""Control changes of running streams (solo_batch_update_streams): rate, DTX and useMDIndex change between two calls and nothing else of
the stream does.  The oracle is the compiled reference with the same values written into its handle at the same packet boundaries
(tests/ref_ctl_poke.py): payloads and lengths byte-exact, PCM sample-exact, DTX records concealed as lost packets as in
test_gpu_stream_ctrl.py."""
import ctypes as C

import numpy as np
import pytest

import ref_ctl_poke as K
import refcodec as R
import solo_testlib as T
from solo_amd.synth import EDGE_FAMILIES, edge_stream

pytestmark = pytest.mark.gpu
need_ref = pytest.mark.skipif(not R.have_ref("fix"), reason="oracle/_ref not present on this box")

I32_MAX = 2 ** 31 - 1
KNOTS_NB = (8000, 9000, 11000, 13000, 16000, 22000)     # TargetRate_table_NB[1..6]: the whole-rate table at k, per description at 2k
KNOTS_WB = (11000, 14000, 17000, 21000, 26000, 36000)
LOW = (1, 6599, 6600)                                   # SILK rates 5000 (clamped up from -1599), 4999 (clamped), 5000
HIGH = (I32_MAX, 101601, 150000)                        # SILK rate clamped down to 100000 (101601: 100001)


def _uniq(v):
    return list(dict.fromkeys(v))


# every NB knot +-1, as the whole rate and as the per-description half, the clamps and <= 0 (= 15600)
RATES_NB = _uniq([0, -5] + list(LOW) + [1600 + m * k + d for k in KNOTS_NB for m in (1, 2) for d in (-1, 0, 1)] + list(HIGH))
RATES_32 = _uniq([0, 15600, 15601] + [1600 + m * k + d for k in KNOTS_WB for m in (1, 2) for d in (-1, 0, 1) if m * k + d >= 14000] + [I32_MAX])
RATES_32_JOINT = [14800, 14801, 22800, 36801, 101600, I32_MAX]
CALLS = (1, 2, 3, 4, 1, 3, 2, 4, 1, 3)                    # packets per call: 24


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _signal(fam, P, samples, seed0, quiet=(4, 10)):
    """fam < EDGE_FAMILIES: that edge family; otherwise speech-like with a near-silent stretch (DTX fires there)"""
    n = P * samples
    if samples == 1280:
        x = T.synth_stream_32k(seed0 + fam, P).reshape(-1) if fam >= EDGE_FAMILIES else edge_stream(seed0 * EDGE_FAMILIES + fam, -(-n // 640)).reshape(-1)[:n]
    elif fam < EDGE_FAMILIES:
        x = edge_stream(seed0 * EDGE_FAMILIES + fam, -(-n // 640)).reshape(-1)[:n]
    else:
        x = R.synth_stream(seed0 + fam, -(-n // 640)).reshape(-1)[:n]
    x = x.copy()
    if fam >= EDGE_FAMILIES and quiet:
        rng = np.random.default_rng(seed0 + fam)
        a, e = min(quiet[0] * samples, n), min(quiet[1] * samples, n)
        x[a:e] = (rng.standard_normal(e - a) * 3).astype(np.int16)
    return np.ascontiguousarray(x.reshape(P, samples))


def _ref_call(pl, n0, n1, m):
    """the decoder call the batched API makes of one record: an empty (DTX) record is concealed as lost"""
    if n0 == 0:
        return b"", 16, 0, 1
    return R.map_loss(pl, n0, n1, not (m & 1), not (m & 2))


def _bounds(calls):
    b = [0]
    for c in calls:
        b.append(b[-1] + c)
    return b


class Plan:
    """N streams, calls of calls[c] packets; before call c stream i takes the control ctl[c][i] = (rate, dtx, md) (None: no update of
    that stream before that call).  ref() drives a poked compiled reference per stream; run() the GPU handle."""

    def __init__(self, pcm, recv, calls, ctl, kw=None):
        self.pcm, self.recv, self.calls, self.ctl, self.kw = pcm, recv, calls, ctl, dict(kw or {})
        self.N, self.P = pcm.shape[:2]
        assert sum(calls) == self.P
        self._ref = None

    def ref(self):
        if self._ref is None:
            kw = self.kw
            enc = [[None] * self.P for _ in range(self.N)]
            pcm = np.zeros(self.pcm.shape, np.int16)
            b = _bounds(self.calls)
            for i in range(self.N):
                e = K.PokeEncoder("fix", rate=kw.get("rate", 13600), joint=kw.get("joint", 0), samplerate=kw.get("samplerate", 16000),
                                  framesize_ms=kw.get("framesize_ms", 40))
                d = K.PokeDecoder("fix", joint=kw.get("joint", 0), samplerate=kw.get("samplerate", 16000), framesize_ms=kw.get("framesize_ms", 40))
                for c in range(len(self.calls)):
                    if self.ctl[c][i] is not None:
                        r, x, m = self.ctl[c][i]
                        e.set_control(rate=r, dtx=x, use_md_index=m)
                        d.set_control(use_md_index=m)
                    for p in range(b[c], b[c + 1]):
                        enc[i][p] = e.encode(self.pcm[i, p])
                        y, ret = d.decode(*_ref_call(*enc[i][p], int(self.recv[i, p])))
                        assert ret == 0
                        pcm[i, p] = y
            self._ref = enc, pcm
        return self._ref

    def run(self, torch, b):
        bs, ns, os_ = [], [], []
        bd = _bounds(self.calls)
        for c in range(len(self.calls)):
            upd = [i for i in range(self.N) if self.ctl[c][i] is not None]
            if upd:
                b.update_streams(upd, rate=[self.ctl[c][i][0] for i in upd], dtx=[self.ctl[c][i][1] for i in upd],
                                 use_md_index=[self.ctl[c][i][2] for i in upd])
            bits, nb, st = b.encode(_dev(self.pcm[:, bd[c]:bd[c + 1]]))
            out, st2 = b.decode(bits, nb, _dev(self.recv[:, bd[c]:bd[c + 1]]))
            torch.cuda.synchronize()
            assert int(st.abs().max()) == 0 and int(st2.abs().max()) == 0, c
            bs.append(bits.cpu().numpy())
            ns.append(nb.cpu().numpy())
            os_.append(out.cpu().numpy())
        return np.concatenate(bs, 1), np.concatenate(ns, 1), np.concatenate(os_, 1)

    def check(self, hb, hn, ho, streams=None):
        enc, pcm = self.ref()
        for i in range(self.N) if streams is None else streams:
            for p in range(self.P):
                pl, n0, n1 = enc[i][p]
                assert (int(hn[i, p, 0]), int(hn[i, p, 1])) == (n0, n1), (i, p)
                assert hb[i, p, :n0].tobytes() == pl[:n0], (i, p)
                assert np.array_equal(ho[i, p], pcm[i, p]), (i, p)


def _schedule(N, n_calls, rates, low, high, seed, fixed=None):
    """per stream its own rate sequence: a low clamp and a high clamp in turn with the other rates in between (every knot is crossed
    both ways), every stream's sequence shifted; DTX / useMDIndex per stream from `fixed` (i -> (dtx, md)) or switching every call"""
    rng = np.random.default_rng(seed)
    ctl = [[None] * N for _ in range(n_calls)]
    for i in range(N):
        mids = list(rng.permutation(rates))
        for c in range(n_calls):
            r = (low[(i + c) % len(low)] if c % 3 == 1 else high[(i + c) % len(high)] if c % 3 == 2 else int(mids[(i + c) % len(mids)]))
            dtx, md = fixed[i] if fixed else ((i + c) % 2, ((i // 2) + c // 2) % 2)
            ctl[c][i] = (int(r), dtx, md)
    return ctl


_PLANS = {}


def _rate_plan():
    if "nb" not in _PLANS:
        fams = list(range(EDGE_FAMILIES)) + [EDGE_FAMILIES, EDGE_FAMILIES + 1]
        N, P = 64, sum(CALLS)
        sig = [i % len(fams) for i in range(N)]
        sigs = [_signal(f, P, 640, 310) for f in fams]
        pcm = np.stack([sigs[s] for s in sig])
        fixed = {i: ((sig[i] + 1) % 2, (sig[i] // 2) % 2) for i in range(N)}
        ctl = _schedule(N, len(CALLS), RATES_NB, LOW, HIGH, 311, fixed)
        # every knot +-1 and every clamp is some stream's rate at some call
        assert set(RATES_NB) <= {ctl[c][i][0] for c in range(len(CALLS)) for i in range(N)}
        _PLANS["nb"] = Plan(pcm, T.bernoulli_recv(N, P, 0.3, 312), CALLS, ctl)
    return _PLANS["nb"]


@need_ref
@pytest.mark.parametrize("knobs", [{}, {"SOLO_DEC_SPLIT": "0"}])
def test_rate_schedules_vs_reference(torch_cuda, monkeypatch, knobs):
    import solo_amd
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)                                        # read at a handle's first decode
    pl = _rate_plan()
    b = solo_amd.SoloBatch(pl.N, encoder=True, decoder=True, slot_bytes=1024)
    hb, hn, ho = pl.run(torch_cuda, b)
    pl.check(hb, hn, ho)


@need_ref
def test_dtx_switched_on_and_off_mid_stream(torch_cuda):
    import solo_amd
    calls = (2, 2, 2, 4, 4, 4, 4)                                        # boundaries 0 2 4 6 10 14 18 22
    N, P = 8, sum(calls)
    rng = np.random.default_rng(320)
    pcm = np.stack([R.synth_stream(320 + i, P) for i in range(N)])
    pcm[:, 6:18] = (rng.standard_normal((N, 12, 640)) * 3).astype(np.int16)    # a quiet stretch of 12 packets
    on = {0: 6, 1: 10, 4: 6, 5: 10}                                      # DTX on at the start of the silence / in its middle
    off = {2: 14, 6: 14}                                                 # on from the start, off in the middle of the silence
    ctl = [[None] * N for _ in calls]
    b_ = _bounds(calls)
    for c in range(len(calls)):
        for i in range(N):
            p = b_[c]
            dtx = (i in on and p >= on[i]) or (i in off and p < off[i])
            ctl[c][i] = (13600 if i < 4 else 24000, int(dtx), 0)         # every stream is updated before every call, most to what it has
    pl = Plan(pcm, T.bernoulli_recv(N, P, 0.2, 321), calls, ctl)
    b = solo_amd.SoloBatch(N, encoder=True, decoder=True, slot_bytes=512)
    hb, hn, ho = pl.run(torch_cuda, b)
    pl.check(hb, hn, ho)
    for i in (1, 5):                                                     # switched on when the silence was long under way: the very
        assert int(hn[i, 10, 0]) == 0, i                                 # next packet is not sent
    for i in (0, 4):
        assert int((hn[i, 6:18, 0] == 0).sum()) > 0, i                   # DTX fires in the silence ...
    for i in (2, 6):
        assert int((hn[i, 14:, 0] == 0).sum()) == 0 and int((hn[i, 6:14, 0] == 0).sum()) > 0, i
    assert int((hn[[3, 7], :, 0] == 0).sum()) == 0                       # ... and never without it


@need_ref
def test_md_index_switch_through_decode(torch_cuda):
    import solo_amd
    calls = (3, 3, 2, 4)
    N, P = 6, sum(calls)
    pcm = np.stack([R.synth_stream(330 + i, P) for i in range(N)])
    start = [0, 0, 1, 1, 0, 1]
    switch = {0: 3, 1: 6, 2: 3, 3: 8}                                    # sender and receiver switch at the same packet
    ctl = [[None] * N for _ in calls]
    b_ = _bounds(calls)
    for c in range(len(calls)):
        for i in range(N):
            md = start[i] ^ (1 if i in switch and b_[c] >= switch[i] else 0)
            if c == 0 or (i in switch and b_[c] == switch[i]):
                ctl[c][i] = (13600, 0, md)
    pl = Plan(pcm, T.bernoulli_recv(N, P, 0.3, 331), calls, ctl)
    b = solo_amd.SoloBatch(N, encoder=True, decoder=True, slot_bytes=512)
    hb, hn, ho = pl.run(torch_cuda, b)
    pl.check(hb, hn, ho)


def _arrivals(rows_of, seq_of, desc_known):
    """all descriptions of the given (stream, packet, (payload, n0, n1)) as arrivals: int32 [n, 5] + the byte pool"""
    rows, pool = [], bytearray()
    for i, p, (pl, n0, n1) in rows_of:
        for dsc, part in ((0, pl[:n0 - n1]), (1, pl[n0 - n1:n0])):
            rows.append((i, seq_of(i, p), dsc if desc_known(i, p) else -1, len(pool), len(part)))
            pool += part
    return np.array(rows, np.int32), np.frombuffer(bytes(pool), np.uint8).copy()


@need_ref
def test_md_index_switch_through_the_receiver_ring(torch_cuda):
    """desc = -1 arrivals are filed by the stream's decoder useMDIndex at insert time: before the receiver switches they are bad"""
    import solo_amd
    torch = torch_cuda
    N, P, H = 4, 10, 4
    pcm = np.stack([R.synth_stream(340 + i, P) for i in range(N)])
    sw = [0, 1, 2]                                                       # stream 3 stays at useMDIndex 0
    payload = []
    for i in range(N):
        e = K.PokeEncoder("fix")
        row = []
        for p in range(P):
            if p == H and i in sw:
                e.set_control(rate=13600, dtx=0, use_md_index=1)
            row.append(e.encode(pcm[i, p]))
        payload.append(row)
    b = solo_amd.SoloBatch(N, encoder=False, decoder=True, slot_bytes=512)
    b.recv_create(16, 256, 0)
    arr, pool = _arrivals([(i, p, payload[i][p]) for i in range(N) for p in range(H)], lambda i, p: p, lambda i, p: True)
    b.recv_insert(_dev(arr), _dev(pool))
    out1, st1 = b.recv_decode(H)
    early, epool = _arrivals([(i, H, payload[i][H]) for i in (0, 1)], lambda i, p: p, lambda i, p: False)
    b.recv_insert(_dev(early), _dev(epool))                              # the receiver has not switched yet
    s = b.recv_stats()
    assert s["inserted"] == 2 * H * N and s["bad"] == 4, s
    b.update_streams(sw, use_md_index=1)
    arr, pool = _arrivals([(i, p, payload[i][p]) for i in range(N) for p in range(H, P)], lambda i, p: p, lambda i, p: i not in sw)
    b.recv_insert(_dev(arr), _dev(pool))
    s = b.recv_stats()
    assert s["inserted"] == 2 * P * N and s["bad"] == 4 and s["duplicate"] == 0, s
    out2, st2 = b.recv_decode(P - H)
    torch.cuda.synchronize()
    assert int(st1.abs().max()) == 0 and int(st2.abs().max()) == 0
    out = np.concatenate([out1.cpu().numpy(), out2.cpu().numpy()], axis=1)
    for i in range(N):
        d = K.PokeDecoder("fix")
        for p in range(P):
            if p == H and i in sw:
                d.set_control(use_md_index=1)
            y, ret = d.decode(*payload[i][p], 4)
            assert ret == 0 and np.array_equal(out[i, p], y), (i, p)


MODES = {
    "32k": (dict(samplerate=32000, rate=15600), RATES_32, (15600, 15601, 17601), (I32_MAX, 101601, 73601)),
    "32k_joint": (dict(samplerate=32000, rate=14800, joint=1), RATES_32_JOINT, (14800, 14801), (I32_MAX, 101600)),
    "joint": (dict(joint=1), RATES_NB, LOW, HIGH),
    "20ms": (dict(framesize_ms=20), RATES_NB, LOW, HIGH),
}


@need_ref
@pytest.mark.parametrize("mode", sorted(MODES))
def test_other_modes_vs_reference(torch_cuda, mode):
    import solo_amd
    kw, rates, low, high = MODES[mode]
    calls = (3, 1, 4, 2, 2)
    N, P = 16, sum(calls)
    samples = 1280 if kw.get("samplerate") == 32000 else (320 if kw.get("framesize_ms") == 20 else 640)
    fams = [0, 3, 7, 11, EDGE_FAMILIES, EDGE_FAMILIES + 1, EDGE_FAMILIES + 2, EDGE_FAMILIES + 3]
    pcm = np.stack([_signal(fams[i % len(fams)], P, samples, 350, quiet=(2, 8)) for i in range(N)])
    ctl = _schedule(N, len(calls), rates, low, high, 351)               # DTX and useMDIndex switch too (both sides at the same packet)
    pl = Plan(pcm, T.bernoulli_recv(N, P, 0.3, 352), calls, ctl, kw)
    create = {k: v for k, v in kw.items()}
    b = solo_amd.SoloBatch(N, encoder=True, decoder=True, slot_bytes=1024, **create)
    hb, hn, ho = pl.run(torch_cuda, b)
    pl.check(hb, hn, ho)


COMBOS = [(r, d, m) for r in (13600, 15600, 24000) for d in (0, 1) for m in (0, 1)]


def _run(torch, b, pcm, recv):
    bits, nb, st = b.encode(_dev(pcm))
    out, st2 = b.decode(bits, nb, _dev(recv))
    torch.cuda.synchronize()
    assert int(st.abs().max()) == 0 and int(st2.abs().max()) == 0
    return bits.cpu().numpy(), nb.cpu().numpy(), out.cpu().numpy()


@need_ref
def test_identity_isolation_and_no_reinitialisation(torch_cuda):
    """(a) an update to the control a stream has is no call at all; (b) unlisted streams are those of a handle that never saw the
    update; (c) an update is not a reset: the same control given by solo_batch_reset_streams gives other outputs"""
    import solo_amd
    torch = torch_cuda
    N, P, H = 16, 10, 5
    rng = np.random.default_rng(360)
    pcm = np.stack([R.synth_stream(360 + i, P) for i in range(N)])
    pcm[:, 3:7] = (rng.standard_normal((N, 4, 640)) * 3).astype(np.int16)
    recv = T.bernoulli_recv(N, P, 0.2, 361)
    ctl0 = [COMBOS[i % len(COMBOS)] for i in range(N)]
    same = list(range(0, N, 2))
    moved = [1, 5, 9, 13]
    new = dict(rate=[24000, 9000, 40000, 15600], dtx=[1, 0, 1, 1], use_md_index=[1, 1, 0, 0])
    hs = []
    for kind in ("update", "none", "reset"):
        b = solo_amd.SoloBatch(N, encoder=True, decoder=True, slot_bytes=512)
        b.reset_streams(range(N), rate=[c[0] for c in ctl0], dtx=[c[1] for c in ctl0], use_md_index=[c[2] for c in ctl0])
        h1 = _run(torch, b, pcm[:, :H], recv[:, :H])
        if kind == "update":
            b.update_streams(same, rate=[ctl0[i][0] for i in same], dtx=[ctl0[i][1] for i in same], use_md_index=[ctl0[i][2] for i in same])
            b.update_streams(moved, **new)
        elif kind == "reset":
            b.reset_streams(moved, **new)
        h2 = _run(torch, b, pcm[:, H:], recv[:, H:])
        hs.append([np.concatenate([x, y], axis=1) for x, y in zip(h1, h2)])
        b.close()
    upd, none, rst = hs
    others = [i for i in range(N) if i not in moved]
    for x, y in zip(upd, none):
        assert np.array_equal(x[others], y[others])                     # (a) + (b): bit for bit
        assert np.array_equal(x[moved, :H], y[moved, :H])
    for k, i in enumerate(moved):                                        # (c) and the updated streams against the poked reference
        assert not (np.array_equal(upd[0][i, H:], rst[0][i, H:]) and np.array_equal(upd[2][i, H:], rst[2][i, H:])), i
        e = K.PokeEncoder("fix", rate=ctl0[i][0], dtx=ctl0[i][1], use_md_index=ctl0[i][2])
        d = K.PokeDecoder("fix", use_md_index=ctl0[i][2])
        for p in range(P):
            if p == H:
                e.set_control(rate=new["rate"][k], dtx=new["dtx"][k], use_md_index=new["use_md_index"][k])
                d.set_control(use_md_index=new["use_md_index"][k])
            pl, n0, n1 = e.encode(pcm[i, p])
            assert (int(upd[1][i, p, 0]), int(upd[1][i, p, 1])) == (n0, n1) and upd[0][i, p, :n0].tobytes() == pl[:n0], (i, p)
            y, ret = d.decode(*_ref_call(pl, n0, n1, int(recv[i, p])))
            assert ret == 0 and np.array_equal(upd[2][i, p], y), (i, p)


@need_ref
@pytest.mark.parametrize("path", ["same_stream", "other_stream", "persist"])
def test_update_behind_an_encode_in_flight(torch_cuda, monkeypatch, path):
    """async joins: the update is issued right behind an encode that may still run; that call's packets keep the old control, the
    next call's packets have the new one"""
    import solo_amd
    torch = torch_cuda
    if path == "persist":
        monkeypatch.setenv("SOLO_ENC_PERSIST", "1")                     # read at the handle's first encode
    N, P, H = 64, 8, 4
    pcm = np.stack([R.synth_stream(370 + i, P) for i in range(N)])
    recv = T.bernoulli_recv(N, P, 0.2, 371)
    b = solo_amd.SoloBatch(N, encoder=True, decoder=True, slot_bytes=512)
    b.set_async_join(True)
    upd = list(range(0, N, 2))
    new = dict(rate=40000, dtx=1, use_md_index=1)
    x1, x2, r1, r2 = _dev(pcm[:, :H]), _dev(pcm[:, H:]), _dev(recv[:, :H]), _dev(recv[:, H:])
    torch.cuda.synchronize()
    bits1, nb1, _ = b.encode(x1)
    if path == "other_stream":
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            b.update_streams(upd, which="enc", **new)
        torch.cuda.current_stream().wait_stream(side)
    else:
        b.update_streams(upd, which="enc", **new)
    bits2, nb2, _ = b.encode(x2)
    b.wait_encode(0)
    out1, _ = b.decode(bits1, nb1, r1)
    b.update_streams(upd, which="dec", use_md_index=1)
    out2, _ = b.decode(bits2, nb2, r2)
    torch.cuda.synchronize()
    hb = np.concatenate([bits1.cpu().numpy(), bits2.cpu().numpy()], axis=1)
    hn = np.concatenate([nb1.cpu().numpy(), nb2.cpu().numpy()], axis=1)
    ho = np.concatenate([out1.cpu().numpy(), out2.cpu().numpy()], axis=1)
    ctl = [[(13600, 0, 0)] * N, [(40000, 1, 1) if i in upd else None for i in range(N)]]
    Plan(pcm, recv, (H, P - H), ctl).check(hb, hn, ho)


@need_ref
def test_update_with_subset_calls(torch_cuda):
    """updates of streams that the next encode_streams / recv_decode_streams list, and of streams they do not: a stream's new control
    applies to its next listed packet"""
    import solo_amd
    torch = torch_cuda
    N, ticks = 16, 8
    pcm = np.stack([R.synth_stream(380 + i, 16) for i in range(N)])
    b = solo_amd.SoloBatch(N, encoder=True, decoder=True, slot_bytes=512)
    b.recv_create(16, 256, 0)
    refs = [(K.PokeEncoder("fix"), K.PokeDecoder("fix")) for _ in range(N)]
    k = [0] * N                                                          # next packet (= sequence number) of every stream
    for t in range(ticks):
        if t % 2 == 0:                                                   # updates: some streams listed by this tick, some not
            upd = [i for i in range(N) if (i + t) % 4 == 0]
            ctl = [(9000 + 4000 * ((i + t) % 7), 0, (i + t // 2) % 2) for i in upd]
            b.update_streams(upd, rate=[c[0] for c in ctl], dtx=0, use_md_index=[c[2] for c in ctl])
            for i, c in zip(upd, ctl):
                refs[i][0].set_control(rate=c[0], dtx=0, use_md_index=c[2])
                refs[i][1].set_control(use_md_index=c[2])
        lst = [i for i in range(N) if (i * 3 + t) % 5 not in (0, 3)]
        P = 1 + t % 2
        x = np.stack([pcm[i, k[i]:k[i] + P] for i in lst])
        bits, nb, st = b.encode(_dev(x), streams=lst)
        torch.cuda.synchronize()
        assert int(st.abs().max()) == 0
        hb, hn = bits.cpu().numpy(), nb.cpu().numpy()
        pay = {}
        for r, i in enumerate(lst):
            for p in range(P):
                pl, n0, n1 = refs[i][0].encode(x[r, p])
                assert (int(hn[r, p, 0]), int(hn[r, p, 1])) == (n0, n1) and hb[r, p, :n0].tobytes() == pl[:n0], (t, i, p)
                pay[(i, p)] = (pl, n0, n1)
        arr, pool = _arrivals([(i, p, pay[(i, p)]) for i in lst for p in range(P)], lambda i, p: k[i] + p, lambda i, p: True)
        b.recv_insert(_dev(arr), _dev(pool))
        out, st2 = b.recv_decode(P, streams=lst)
        torch.cuda.synchronize()
        assert int(st2.abs().max()) == 0
        out = out.cpu().numpy()
        for r, i in enumerate(lst):
            for p in range(P):
                y, ret = refs[i][1].decode(*pay[(i, p)], 4)
                assert ret == 0 and np.array_equal(out[r, p], y), (t, i, p)
            k[i] += P


def _enc_ctrls(n, **over):
    import solo_amd
    arr = (solo_amd.USER_Ctrl_enc * n)()
    for i in range(n):
        c = solo_amd.default_enc_ctrl()
        for key, v in over.items():
            setattr(c, key, v)
        arr[i] = c
    return arr


def _dec_ctrls(n, **over):
    import solo_amd
    arr = (solo_amd.USER_Ctrl_dec * n)()
    for i in range(n):
        c = solo_amd.default_dec_ctrl()
        for key, v in over.items():
            setattr(c, key, v)
        arr[i] = c
    return arr


def test_refused_calls_change_nothing(torch_cuda):
    """every call solo_batch_reset_streams refuses is refused here too (-1), and later outputs are those of a handle that never made it"""
    import solo_amd
    torch = torch_cuda
    N, P, H = 8, 6, 3
    pcm = np.stack([R.synth_stream(390 + i, P) for i in range(N)])
    recv = T.bernoulli_recv(N, P, 0.2, 391)
    ix = lambda *v: (C.c_int32 * len(v))(*v)
    refused = [
        (ix(0, N), 2, 3, None, None),                                   # index out of range
        (ix(-1), 1, 3, None, None),
        (ix(1, 1), 2, 3, None, None),                                   # listed twice
        (ix(0), 0, 3, None, None),                                      # n <= 0
        (ix(*range(N)), N + 1, 3, None, None),                          # n > N
        (ix(0), 1, 0, None, None),                                      # which
        (ix(0), 1, 4, None, None),
        (ix(0), 1, 1, _enc_ctrls(1, samplerate=32000, targetRate_bps=24000), None),
        (ix(0), 1, 1, _enc_ctrls(1, framesize_ms=20), None),
        (ix(0), 1, 1, _enc_ctrls(1, joint_enable=1, joint_mode=1), None),
        (ix(0), 1, 2, None, _dec_ctrls(1, samplerate=32000)),
        (ix(0), 1, 2, None, _dec_ctrls(1, framesize_ms=20)),
        (ix(0), 1, 2, None, _dec_ctrls(1, joint_enable=1, joint_mode=1)),
        (ix(0), 1, 2, _enc_ctrls(1), None),                             # an encoder control in a decoder-only call
        (ix(0), 1, 1, None, _dec_ctrls(1)),                             # a decoder control in an encoder-only call
        (ix(0, 3), 2, 3, _enc_ctrls(2, useMDIndex=1, targetRate_bps=40000), _dec_ctrls(2, framesize_ms=20)),   # one bad control refuses all
    ]
    outs = []
    for twin in (False, True):
        b = solo_amd.SoloBatch(N, encoder=True, decoder=True, slot_bytes=512)
        h1 = _run(torch, b, pcm[:, :H], recv[:, :H])
        if not twin:
            for args in refused:
                assert b.lib.solo_batch_update_streams(b.h, *args, b._stream()) == -1, args[1:3]
            for bad in (dict(streams=[0, N]), dict(streams=[2, 2]), dict(streams=[]), dict(streams=[0], rate=[1, 2])):
                with pytest.raises(ValueError):
                    b.update_streams(**bad)
        h2 = _run(torch, b, pcm[:, H:], recv[:, H:])
        outs.append([np.concatenate([x, y], axis=1) for x, y in zip(h1, h2)])
    for x, y in zip(*outs):
        assert np.array_equal(x, y)

    # 32 kHz: a rate that leaves SILK below 14 kbps is refused, the handle goes on as its twin
    x32 = np.stack([T.synth_stream_32k(392 + i, 4) for i in range(2)])
    r32 = np.full((2, 4), 3, np.uint8)
    outs = []
    for twin in (False, True):
        w = solo_amd.SoloBatch(2, rate=15600, encoder=True, decoder=True, slot_bytes=512, samplerate=32000)
        g1 = _run(torch, w, x32[:, :2], r32[:, :2])
        if not twin:
            assert w.lib.solo_batch_update_streams(w.h, ix(1), 1, 1, _enc_ctrls(1, samplerate=32000, targetRate_bps=13600), None, w._stream()) == -1
            assert w.lib.solo_batch_update_streams(w.h, ix(0), 1, 1, _enc_ctrls(1, samplerate=32000, targetRate_bps=15599), None, w._stream()) == -1
            with pytest.raises(ValueError):
                w.update_streams([1], rate=13600)
        g2 = _run(torch, w, x32[:, 2:], r32[:, 2:])
        outs.append([np.concatenate([x, y], axis=1) for x, y in zip(g1, g2)])
    for x, y in zip(*outs):
        assert np.array_equal(x, y)

    # decoder-only handle: an encoder control, or the encoder direction, is refused
    d = solo_amd.SoloBatch(2, encoder=False, decoder=True, slot_bytes=512)
    assert d.lib.solo_batch_update_streams(d.h, ix(0), 1, 3, _enc_ctrls(1), None, d._stream()) == -1
    assert d.lib.solo_batch_update_streams(d.h, ix(0), 1, 1, None, None, d._stream()) == -1
    assert d.lib.solo_batch_update_streams(d.h, ix(0), 1, 2, _enc_ctrls(1), None, d._stream()) == -1
    assert d.lib.solo_batch_update_streams(d.h, ix(0), 1, 2, None, _dec_ctrls(1, useMDIndex=1), d._stream()) == 0
    with pytest.raises(ValueError):
        d.update_streams([0], rate=24000)

"""Subset calls of a batch handle (solo_batch_encode_streams, solo_batch_decode_streams, solo_recv_decode_streams): only the listed
streams are encoded / decoded / played out, the others keep their state bit for bit.  Every stream is compared with a compiled-reference
encoder / decoder that is driven only on the calls where its stream was listed: payloads and lengths byte-exact, PCM sample-exact."""
import ctypes as C

import numpy as np
import pytest

import refcodec as R
import solo_testlib as T

pytestmark = pytest.mark.gpu
need_ref = pytest.mark.skipif(not R.have_ref("fix"), reason="oracle/_ref not present on this box")

COMBOS = [(r, d, m) for r in (13600, 15600, 24000) for d in (0, 1) for m in (0, 1)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _pcm(N, T_, seed0, quiet=(), samples=640):
    """per-stream packet sequences [N, T_, samples], speech-like, near-silent over the packet ranges in `quiet` (DTX fires there)"""
    rng = np.random.default_rng(seed0)
    if samples == 1280:
        x = np.stack([T.synth_stream_32k(seed0 + i, T_) for i in range(N)])
    else:
        k = -(-T_ * samples // 640)
        x = np.stack([R.synth_stream(seed0 + i, k).reshape(-1)[:T_ * samples].reshape(T_, samples) for i in range(N)])
    for a, e in quiet:
        x[:, a:e] = (rng.standard_normal((N, e - a, samples)) * 3).astype(np.int16)
    return x


def _ref_call(pl, n0, n1, m):
    """the decoder call the batched API makes of one record: an empty (DTX) record is concealed as lost"""
    if n0 == 0:
        return b"", 16, 0, 1
    return R.map_loss(pl, n0, n1, not (m & 1), not (m & 2))


class _Ref:
    """one stream's compiled-reference encoder + decoder with its own control"""

    def __init__(self, rate=13600, dtx=0, md=0, **kw):
        self.e = R.RefEncoder("fix", rate=rate, dtx=dtx, use_md_index=md, **kw)
        self.d = R.RefDecoder("fix", use_md_index=md, **kw)

    def step(self, x, m):
        pl, n0, n1 = self.e.encode(x)
        y, ret = self.d.decode(*_ref_call(pl, n0, n1, m))
        assert ret == 0
        return (pl[:n0], n0, n1), y


def _run_schedule(torch, b, x, recv, calls, decode=True, tensor_lists=False):
    """calls: [(streams or None = a plain full call, P)].  Every listed stream takes the next P packets of its own sequence x[i].
    Returns, per stream, what it got in order: encoder records (payload, n0, n1) and decoded packets."""
    N = x.shape[0]
    pos = np.zeros(N, np.int64)
    enc = [[] for _ in range(N)]
    dec = [[] for _ in range(N)]
    for k, (lst, P) in enumerate(calls):
        rows = list(range(N)) if lst is None else [int(i) for i in lst]
        if not rows:
            continue
        pcm = np.stack([x[i, pos[i]:pos[i] + P] for i in rows])
        rv = np.stack([recv[i, pos[i]:pos[i] + P] for i in rows])
        kw = {}
        if lst is not None:
            kw["streams"] = torch.tensor(rows, dtype=torch.int32, device="cuda") if (tensor_lists and k % 2) else rows
        bits, nb, st = b.encode(_dev(pcm), **kw)
        if decode:
            out, st2 = b.decode(bits, nb, _dev(rv), **kw)
        torch.cuda.synchronize()
        assert int(st.abs().max()) == 0, (k, st.cpu().numpy())
        hb, hn = bits.cpu().numpy(), nb.cpu().numpy()
        if decode:
            assert int(st2.abs().max()) == 0, (k, st2.cpu().numpy())
            ho = out.cpu().numpy()
        for r, i in enumerate(rows):
            for p in range(P):
                n0 = int(hn[r, p, 0])
                enc[i].append((hb[r, p, :n0].tobytes(), n0, int(hn[r, p, 1])))
                if decode:
                    dec[i].append(ho[r, p])
        pos[rows] += P
    return enc, dec, pos


def _check(x, recv, enc, dec, refs):
    for i, ref in refs.items():
        assert len(enc[i]) > 0 or len(dec[i]) == 0
        for p in range(len(enc[i])):
            e, y = ref.step(x[i, p], int(recv[i, p]))
            assert enc[i][p] == e, (i, p, enc[i][p][1:], e[1:])
            if dec[i]:
                assert np.array_equal(dec[i][p], y), (i, p)


def _sparse_calls(N, ticks, seed, p3_every=5):
    """ticks of random subsets (0 - 100 % of the streams; one tick lists nothing, one lists everything), P = 3 on some ticks"""
    rng = np.random.default_rng(seed)
    calls = []
    for t in range(ticks):
        frac = 0.0 if t == 4 else (1.0 if t == 9 else rng.random())
        lst = np.flatnonzero(rng.random(N) < frac) if frac < 1.0 else np.arange(N)
        calls.append((lst, 3 if t % p3_every == 2 else 1))
    return calls


def _need(calls, N, tail=0):
    c = np.zeros(N, np.int64)
    for lst, P in calls:
        c[np.arange(N) if lst is None else np.asarray(lst, np.int64)] += P
    return int(c.max()) + tail


@need_ref
@pytest.mark.parametrize("path", ["split", "single_kernel"])
def test_sparse_schedule_both_directions(torch_cuda, monkeypatch, path):
    import solo_amd
    torch = torch_cuda
    if path == "single_kernel":
        monkeypatch.setenv("SOLO_DEC_SPLIT", "0")                      # read at the handle's first decode
    N = 256
    calls = _sparse_calls(N, 30, 311) + [(None, 2), (None, 1)]
    Tn = _need(calls, N)
    x = _pcm(N, Tn, 12000, quiet=[(4, 9)])
    recv = T.bernoulli_recv(N, Tn, 0.25, 53)
    b = solo_amd.SoloBatch(N, encoder=True, decoder=True, slot_bytes=512)
    ctl = [COMBOS[(i * 7) % len(COMBOS)] for i in range(N)]
    b.reset_streams(range(N), rate=[c[0] for c in ctl], dtx=[c[1] for c in ctl], use_md_index=[c[2] for c in ctl])
    enc, dec, pos = _run_schedule(torch, b, x, recv, calls, tensor_lists=True)
    assert pos.min() >= 3 and pos.max() > pos.min()                     # the streams really moved on by different amounts
    dtx = [i for i in range(N) if ctl[i][1]]
    assert sum(1 for i in dtx for r in enc[i] if r[1] == 0) > 0        # DTX fired
    _check(x, recv, enc, dec, {i: _Ref(*ctl[i]) for i in range(N)})


def test_all_listed_equals_plain_calls(torch_cuda):
    import solo_amd
    torch = torch_cuda
    N, P = 48, 4
    x = _pcm(N, 2 * P, 13000, quiet=[(2, 5)])
    recv = T.bernoulli_recv(N, 2 * P, 0.3, 59)
    outs = []
    for listed in (False, True):
        b = solo_amd.SoloBatch(N, encoder=True, decoder=True, slot_bytes=512)
        ctl = [COMBOS[i % len(COMBOS)] for i in range(N)]
        b.reset_streams(range(N), rate=[c[0] for c in ctl], dtx=[c[1] for c in ctl], use_md_index=[c[2] for c in ctl])
        kw = dict(streams=list(range(N))) if listed else {}
        got = []
        for h in range(2):
            bits, nb, st = b.encode(_dev(x[:, h * P:(h + 1) * P]), **kw)
            out, st2 = b.decode(bits, nb, _dev(recv[:, h * P:(h + 1) * P]), **kw)
            got += [bits.cpu().numpy(), nb.cpu().numpy(), st.cpu().numpy(), out.cpu().numpy(), st2.cpu().numpy()]
        outs.append(got)
    for a, c in zip(*outs):
        assert np.array_equal(a, c)


def test_listed_subset_equals_a_handle_of_that_size(torch_cuda):
    import solo_amd
    torch = torch_cuda
    N, P = 64, 3
    lst = list(range(1, N, 3))
    n = len(lst)
    x = _pcm(n, 3 * P, 14000)
    recv = T.bernoulli_recv(n, 3 * P, 0.3, 61)
    big = solo_amd.SoloBatch(N, encoder=True, decoder=True, slot_bytes=512, use_md_index=1)
    small = solo_amd.SoloBatch(n, encoder=True, decoder=True, slot_bytes=512, use_md_index=1)
    for h in range(3):
        xs, rs = _dev(x[:, h * P:(h + 1) * P]), _dev(recv[:, h * P:(h + 1) * P])
        a = big.encode(xs, streams=lst)
        c = small.encode(xs)
        da = big.decode(a[0], a[1], rs, streams=lst)
        dc = small.decode(c[0], c[1], rs)
        torch.cuda.synchronize()
        for u, v in zip(list(a) + list(da), list(c) + list(dc)):
            assert np.array_equal(u.cpu().numpy(), v.cpu().numpy()), h


@need_ref
@pytest.mark.parametrize("case", ["groups", "around_full_calls", "persist"])
def test_pipeline_corners(torch_cuda, monkeypatch, case):
    import solo_amd
    torch = torch_cuda
    N = 256
    rng = np.random.default_rng(71)
    if case == "groups":
        monkeypatch.setenv("SOLO_ENC_GROUP", "64")                     # read when the handle first encodes
        l200 = np.sort(rng.choice(N, 200, replace=False))
        calls = [(l200, 3), (None, 1), (l200[::3], 2)]
    elif case == "around_full_calls":
        calls = [(None, 3), (np.arange(0, N, 2), 1), (None, 2), (np.arange(0, N, 5), 4), (None, 1)]
    else:
        monkeypatch.setenv("SOLO_ENC_PERSIST", "1")                    # subset calls fall back to the launch-per-chunk schedule
        calls = [(None, 3), (np.arange(1, N, 3), 2), (None, 2), (np.arange(N // 2), 1)]
    Tn = _need(calls, N)
    x = _pcm(N, Tn, 15000)
    recv = T.bernoulli_recv(N, Tn, 0.2, 73)
    b = solo_amd.SoloBatch(N, encoder=True, decoder=True, slot_bytes=512)
    enc, dec, _ = _run_schedule(torch, b, x, recv, calls)
    _check(x, recv, enc, dec, {i: _Ref() for i in range(N)})


@need_ref
def test_async_join_two_subset_calls_in_flight(torch_cuda):
    import solo_amd
    torch = torch_cuda
    N, P = 64, 2
    la, lb = list(range(0, N, 2)), list(range(0, N, 3))
    x = _pcm(N, 2 * P, 16000)
    b = solo_amd.SoloBatch(N, encoder=True, decoder=False, slot_bytes=512)
    b.set_async_join(True)
    pos = {i: 0 for i in range(N)}
    ins = []
    for lst in (la, lb):
        ins.append(_dev(np.stack([x[i, pos[i]:pos[i] + P] for i in lst])))
        for i in lst:
            pos[i] += P
    torch.cuda.synchronize()
    ra = b.encode(ins[0], streams=la)
    rb = b.encode(ins[1], streams=lb)                                   # enqueued while the first call's tail still runs
    b.wait_encode(0)
    b.wait_encode(1)
    got = {i: [] for i in range(N)}
    for lst, (bits, nb, st) in ((la, ra), (lb, rb)):
        hb, hn = bits.cpu().numpy(), nb.cpu().numpy()
        assert int(st.abs().max().cpu()) == 0
        for r, i in enumerate(lst):
            for p in range(P):
                n0 = int(hn[r, p, 0])
                got[i].append((hb[r, p, :n0].tobytes(), n0, int(hn[r, p, 1])))
    for i in range(N):
        e = R.RefEncoder("fix")
        for p, g in enumerate(got[i]):
            pl, n0, n1 = e.encode(x[i, p])
            assert g == (pl[:n0], n0, n1), (i, p)


@need_ref
@pytest.mark.parametrize("mode", ["32k", "20ms", "joint"])
def test_modes(torch_cuda, mode):
    import solo_amd
    torch = torch_cuda
    N = 32
    calls = _sparse_calls(N, 8, 83, p3_every=4) + [(None, 1)]
    Tn = _need(calls, N)
    recv = T.bernoulli_recv(N, Tn, 0.25, 89)
    if mode == "32k":
        kw = dict(samplerate=32000)
        ctl = [((15600, 24000)[i % 2], 0, (i // 2) % 2) for i in range(N)]
        x = _pcm(N, Tn, 17000, samples=1280)
        b = solo_amd.SoloBatch(N, rate=15600, encoder=True, decoder=True, slot_bytes=512, samplerate=32000)
    elif mode == "20ms":
        kw = dict(framesize_ms=20)
        ctl = [COMBOS[(i * 5) % len(COMBOS)] for i in range(N)]
        x = _pcm(N, Tn, 17100, quiet=[(2, 6)], samples=320)
        b = solo_amd.SoloBatch(N, encoder=True, decoder=True, slot_bytes=512, framesize_ms=20)
    else:
        kw = dict(joint=1)
        ctl = None
        x = _pcm(N, Tn, 17200)
        b = solo_amd.SoloBatch(N, encoder=True, decoder=True, slot_bytes=512, joint=1)
    if ctl is not None:
        b.reset_streams(range(N), rate=[c[0] for c in ctl], dtx=[c[1] for c in ctl], use_md_index=[c[2] for c in ctl])
    enc, dec, _ = _run_schedule(torch, b, x, recv, calls)
    _check(x, recv, enc, dec, {i: (_Ref(*ctl[i], **kw) if ctl else _Ref(**kw)) for i in range(N)})


def _arrivals(rows):
    """[(stream, seq, payload record)] -> int32 [n, 5] arrivals (both descriptions, desc known) + the byte pool"""
    out, pool = [], bytearray()
    for i, seq, (pl, n0, n1) in rows:
        for dsc, part in ((0, pl[:n0 - n1]), (1, pl[n0 - n1:n0])):
            out.append((i, seq, dsc, len(pool), len(part)))
            pool += part
    return np.array(out, np.int32), np.frombuffer(bytes(pool), np.uint8).copy()


@need_ref
def test_ring_plays_out_listed_streams_only(torch_cuda):
    import solo_amd
    torch = torch_cuda
    N, P, D = 16, 8, 8
    x = _pcm(N, P, 18000)
    refs = [_Ref(md=1) for _ in range(N)]
    payload = [[refs[i].e.encode(x[i, p]) for p in range(P)] for i in range(N)]
    b = solo_amd.SoloBatch(N, encoder=False, decoder=True, slot_bytes=512, use_md_index=1)
    b.recv_create(D, 256, 0)
    arr, pool = _arrivals([(i, p, payload[i][p]) for i in range(N) for p in range(6)])
    b.recv_insert(_dev(arr), _dev(pool))
    play = np.zeros(N, np.int64)
    got = {i: [] for i in range(N)}

    def play_out(lst, k):
        out, st = b.recv_decode(k, streams=lst)
        o = out.cpu().numpy()
        assert int(st.abs().max().cpu()) == 0 and o.shape[0] == len(lst)
        for r, i in enumerate(lst):
            got[i] += list(o[r])
            play[i] += k

    A, B = list(range(0, N, 2)), [0, 3, 6, 9, 12, 15]
    play_out(A, 2)
    play_out(B, 2)
    play_out(A, 1)
    s0 = b.recv_stats()
    # late / ahead follow each stream's OWN play-out position: stream 0 has played 5 packets, stream 1 none
    late = [(0, 2, payload[0][2])]
    ahead = [(1, D, payload[1][0])]
    rest = [(i, p, payload[i][p]) for i in range(N) for p in (6, 7)]
    arr, pool = _arrivals(rest + late + ahead)
    b.recv_insert(_dev(arr), _dev(pool))
    s1 = b.recv_stats()
    assert s1["inserted"] - s0["inserted"] == 2 * len(rest), (s0, s1)
    assert s1["late"] - s0["late"] == 2 and s1["ahead"] - s0["ahead"] == 2 and s1["duplicate"] == s0["duplicate"], (s0, s1)
    # every stream plays on to the end of its queue: the unlisted ones from where they were left, at their own sequence numbers
    for k in sorted(set(P - play)):
        lst = [i for i in range(N) if P - play[i] == k]
        if k > 0:
            play_out(lst, int(k))
    torch.cuda.synchronize()
    for i in range(N):
        assert len(got[i]) == P
        for p in range(P):
            y, ret = refs[i].d.decode(*payload[i][p], 4)
            assert ret == 0 and np.array_equal(got[i][p], y), (i, p)


@need_ref
def test_refused_lists_change_nothing(torch_cuda):
    import solo_amd
    torch = torch_cuda
    N, H = 8, 3
    x = _pcm(N, 2 * H, 19000)
    recv = T.bernoulli_recv(N, 2 * H, 0.2, 97)
    b = solo_amd.SoloBatch(N, encoder=True, decoder=True, slot_bytes=512)
    lib, stream = b.lib, b._stream()
    enc, dec, _ = _run_schedule(torch, b, x[:, :H], recv[:, :H], [(None, H)])
    bad_lists = [[3, 1], [2, 2], [0, N], [-1, 2]]                     # unsorted, duplicate, out of range, negative
    for bad in bad_lists:
        n = len(bad)
        d_list = torch.tensor(bad, dtype=torch.int32, device="cuda")
        pcm = _dev(x[:n, :1])
        bits = torch.full((n, 1, 512), 0xAB, dtype=torch.uint8, device="cuda")
        nb = torch.full((n, 1, 2), 77, dtype=torch.int16, device="cuda")
        out = torch.full((n, 1, 640), 5, dtype=torch.int16, device="cuda")
        for call in ("enc", "dec"):
            st = torch.full((n,), 7, dtype=torch.int32, device="cuda")
            if call == "enc":
                r = lib.solo_batch_encode_streams(b.h, d_list.data_ptr(), n, pcm.data_ptr(), 1, bits.data_ptr(), nb.data_ptr(), st.data_ptr(), stream)
            else:
                r = lib.solo_batch_decode_streams(b.h, d_list.data_ptr(), n, bits.data_ptr(), nb.data_ptr(), None, 1, out.data_ptr(), st.data_ptr(), stream)
            torch.cuda.synchronize()
            assert r == 0 and st.cpu().tolist() == [-1] * n, (bad, call, st.cpu().tolist())
        assert bool((bits == 0xAB).all()) and bool((nb == 77).all()) and bool((out == 5).all()), bad
    # refused on the host: n <= 0, n > N, NULL pointers
    ok = torch.arange(N, dtype=torch.int32, device="cuda")
    pcm, bits = _dev(x[:, :1]), torch.zeros((N, 1, 512), dtype=torch.uint8, device="cuda")
    nb, out = torch.zeros((N, 1, 2), dtype=torch.int16, device="cuda"), torch.zeros((N, 1, 640), dtype=torch.int16, device="cuda")
    for n in (0, -1, N + 1):
        assert lib.solo_batch_encode_streams(b.h, ok.data_ptr(), n, pcm.data_ptr(), 1, bits.data_ptr(), nb.data_ptr(), None, stream) == -1
        assert lib.solo_batch_decode_streams(b.h, ok.data_ptr(), n, bits.data_ptr(), nb.data_ptr(), None, 1, out.data_ptr(), None, stream) == -1
    assert lib.solo_batch_encode_streams(b.h, None, N, pcm.data_ptr(), 1, bits.data_ptr(), nb.data_ptr(), None, stream) == -1
    assert lib.solo_batch_encode_streams(b.h, ok.data_ptr(), N, None, 1, bits.data_ptr(), nb.data_ptr(), None, stream) == -1
    assert lib.solo_batch_decode_streams(b.h, None, N, bits.data_ptr(), nb.data_ptr(), None, 1, out.data_ptr(), None, stream) == -1
    assert lib.solo_batch_decode_streams(b.h, ok.data_ptr(), N, bits.data_ptr(), nb.data_ptr(), None, 1, None, None, stream) == -1
    assert lib.solo_recv_decode_streams(b.h, ok.data_ptr(), N, 1, out.data_ptr(), None, stream) == -1      # no ring yet
    for bad in (dict(streams=[2, 1]), dict(streams=[1, 1]), dict(streams=[0, N]), dict(streams=[])):
        with pytest.raises(ValueError):
            b.encode(_dev(x[:len(bad["streams"]), :1]) if bad["streams"] else _dev(x[:1, :1]), **bad)
    # the following full calls match references that never saw the refused calls
    enc2, dec2, _ = _run_schedule(torch, b, x[:, H:], recv[:, H:], [(None, H)])
    _check(x, recv, [e + f for e, f in zip(enc, enc2)], [e + f for e, f in zip(dec, dec2)], {i: _Ref() for i in range(N)})

    # receiver ring: a refused play-out moves no play-out position and frees no queue entry
    refs = [_Ref(md=1) for _ in range(4)]
    payload = [[refs[i].e.encode(x[i, p]) for p in range(4)] for i in range(4)]
    d = solo_amd.SoloBatch(4, encoder=False, decoder=True, slot_bytes=512, use_md_index=1)
    d.recv_create(8, 256, 0)
    arr, pool = _arrivals([(i, p, payload[i][p]) for i in range(4) for p in range(4)])
    d.recv_insert(_dev(arr), _dev(pool))
    for bad in ([2, 0], [1, 1], [0, 4], [-2]):
        n = len(bad)
        d_list = torch.tensor(bad, dtype=torch.int32, device="cuda")
        out = torch.full((n, 2, 640), 5, dtype=torch.int16, device="cuda")
        st = torch.full((n,), 7, dtype=torch.int32, device="cuda")
        assert d.lib.solo_recv_decode_streams(d.h, d_list.data_ptr(), n, 2, out.data_ptr(), st.data_ptr(), d._stream()) == 0
        torch.cuda.synchronize()
        assert st.cpu().tolist() == [-1] * n and bool((out == 5).all()), bad
    ok4 = torch.arange(4, dtype=torch.int32, device="cuda")
    assert d.lib.solo_recv_decode_streams(d.h, ok4.data_ptr(), 5, 1, out.data_ptr(), None, d._stream()) == -1
    assert d.lib.solo_recv_decode_streams(d.h, ok4.data_ptr(), 4, 9, out.data_ptr(), None, d._stream()) == -1        # n_packets > depth
    assert d.lib.solo_recv_decode_streams(d.h, ok4.data_ptr(), 4, 1, None, None, d._stream()) == -1
    got, st = d.recv_decode(4)
    torch.cuda.synchronize()
    assert int(st.abs().max().cpu()) == 0
    got = got.cpu().numpy()
    for i in range(4):
        for p in range(4):
            y, ret = refs[i].d.decode(*payload[i][p], 4)
            assert ret == 0 and np.array_equal(got[i, p], y), (i, p)

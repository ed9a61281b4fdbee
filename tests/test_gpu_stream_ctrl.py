"""Per-stream codec control and stream lifecycle in one batch handle (solo_batch_reset_streams, solo_recv_reset_streams).  Every
stream is compared with a compiled-reference encoder / decoder created with THAT stream's control: payloads and lengths byte-exact,
PCM sample-exact."""
import ctypes as C

import numpy as np
import pytest

import refcodec as R
import solo_testlib as T

pytestmark = pytest.mark.gpu
need_ref = pytest.mark.skipif(not R.have_ref("fix"), reason="oracle/_ref not present on this box")

# the 12 control combinations: {13600, 15600, 24000} bps x DTX off / on x useMDIndex 0 / 1
COMBOS = [(r, d, m) for r in (13600, 15600, 24000) for d in (0, 1) for m in (0, 1)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch


def _pcm(N, P, seed0, quiet=(), samples=640):
    """speech-like streams with near-silent stretches (packet ranges in `quiet`) so that DTX fires"""
    rng = np.random.default_rng(seed0)
    if samples == 1280:
        x = np.stack([T.synth_stream_32k(seed0 + i, P) for i in range(N)])
    else:
        x = np.stack([R.synth_stream(seed0 + i, P * samples // 640).reshape(P, samples) for i in range(N)])
    for a, e in quiet:
        x[:, a:e] = (rng.standard_normal((N, e - a, samples)) * 3).astype(np.int16)
    return x


def _ref_call(pl, n0, n1, m):
    """the decoder call the batched API makes of one record: an empty (DTX) record is concealed as lost"""
    if n0 == 0:
        return b"", 16, 0, 1
    return R.map_loss(pl, n0, n1, not (m & 1), not (m & 2))


def _check_enc(hb, hn, i, p, ref):
    pl, n0, n1 = ref
    assert (int(hn[i, p, 0]), int(hn[i, p, 1])) == (n0, n1), (i, p)
    assert hb[i, p, :n0].tobytes() == pl[:n0], (i, p)


def _run(torch, b, pcm, recv):
    bits, nb, st = b.encode(torch.from_numpy(np.ascontiguousarray(pcm)).to(b.device))
    out, st2 = b.decode(bits, nb, torch.from_numpy(np.ascontiguousarray(recv)).to(b.device))
    torch.cuda.synchronize()
    assert int(st.abs().max()) == 0 and int(st2.abs().max()) == 0
    return bits.cpu().numpy(), nb.cpu().numpy(), out.cpu().numpy()


class _Ref:
    """one stream's compiled-reference encoder + decoder with its own control"""

    def __init__(self, rate=13600, dtx=0, md=0, **kw):
        self.e = R.RefEncoder("fix", rate=rate, dtx=dtx, use_md_index=md, **kw)
        self.d = R.RefDecoder("fix", use_md_index=md, **kw)

    def step(self, x, m):
        pl, n0, n1 = self.e.encode(x)
        y, ret = self.d.decode(*_ref_call(pl, n0, n1, m))
        assert ret == 0
        return (pl, n0, n1), y


def _check_streams(hb, hn, ho, recv, pcm, refs, streams, p_off=0):
    for i in streams:
        for p in range(pcm.shape[1]):
            enc, y = refs[i].step(pcm[i, p], int(recv[i, p]))
            _check_enc(hb, hn, i, p + p_off, enc)
            assert np.array_equal(ho[i, p + p_off], y), (i, p)


@need_ref
def test_mixed_control_batch_vs_reference(torch_cuda):
    import solo_amd
    N, P = 512, 12
    pcm = _pcm(N, P, 4100, quiet=[(4, 9)])
    recv = T.bernoulli_recv(N, P, 0.3, 17)
    b = solo_amd.SoloBatch(N, encoder=True, decoder=True, slot_bytes=512)
    ctl = [COMBOS[i % len(COMBOS)] for i in range(N)]
    b.reset_streams(range(N), rate=[c[0] for c in ctl], dtx=[c[1] for c in ctl], use_md_index=[c[2] for c in ctl])
    hb, hn, ho = _run(torch_cuda, b, pcm, recv)
    dtx_streams = [i for i in range(N) if ctl[i][1]]
    assert int((hn[dtx_streams, :, 0] == 0).sum()) > 0                  # DTX fired
    assert int((hn[[i for i in range(N) if not ctl[i][1]], :, 0] == 0).sum()) == 0
    refs = {i: _Ref(*ctl[i]) for i in range(N)}
    _check_streams(hb, hn, ho, recv, pcm, refs, range(N))


_CONT = {}


def _continuing(pcm, recv):
    """the reference of a stream that was never reset: 13600 bps, no DTX, useMDIndex 0, over all packets"""
    key = (pcm.shape, T.md5(pcm), T.md5(recv))
    if key not in _CONT:
        out = []
        for i in range(pcm.shape[0]):
            r = _Ref()
            out.append([r.step(pcm[i, p], int(recv[i, p])) for p in range(pcm.shape[1])])
        _CONT[key] = out
    return _CONT[key]


@need_ref
@pytest.mark.parametrize("path", ["default", "async_join", "persist"])
def test_mid_call_lifecycle(torch_cuda, monkeypatch, path):
    import solo_amd
    torch = torch_cuda
    if path == "persist":
        monkeypatch.setenv("SOLO_ENC_PERSIST", "1")                     # read at the handle's first encode
    N, P, H = 256, 12, 6
    pcm = _pcm(N, P, 5200, quiet=[(8, 11)])
    recv = T.bernoulli_recv(N, P, 0.2, 23)
    b = solo_amd.SoloBatch(N, encoder=True, decoder=True, slot_bytes=512)
    if path == "async_join":
        b.set_async_join(True)
    reset = list(range(0, N, 7))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(b.device)
    x1, x2, r1, r2 = dev(pcm[:, :H]), dev(pcm[:, H:]), dev(recv[:, :H]), dev(recv[:, H:])
    torch.cuda.synchronize()
    new = dict(rate=24000, dtx=1, use_md_index=1)
    bits1, nb1, _ = b.encode(x1)
    if path == "async_join":
        b.reset_streams(reset, which="enc", **new)                      # right behind the encode still in flight
        b.wait_encode(0)
        out1, _ = b.decode(bits1, nb1, r1)
        b.reset_streams(reset, which="dec", use_md_index=1)
    else:
        out1, _ = b.decode(bits1, nb1, r1)
        b.reset_streams(reset, **new)
    bits2, nb2, _ = b.encode(x2)
    if path == "async_join":
        b.wait_encode(0)
    out2, _ = b.decode(bits2, nb2, r2)
    torch.cuda.synchronize()
    hb = np.concatenate([bits1.cpu().numpy(), bits2.cpu().numpy()], axis=1)
    hn = np.concatenate([nb1.cpu().numpy(), nb2.cpu().numpy()], axis=1)
    ho = np.concatenate([out1.cpu().numpy(), out2.cpu().numpy()], axis=1)
    cont = _continuing(pcm, recv)
    rs = set(reset)
    for i in range(N):
        for p in range(P if i not in rs else H):
            enc, y = cont[i][p]
            _check_enc(hb, hn, i, p, enc)
            assert np.array_equal(ho[i, p], y), (i, p)
    refs = {i: _Ref(24000, 1, 1) for i in reset}
    _check_streams(hb, hn, ho, recv[:, H:], pcm[:, H:], refs, reset, p_off=H)


@need_ref
def test_partial_resets_leave_the_other_direction(torch_cuda):
    import solo_amd
    N, P, H = 24, 10, 5
    pcm = _pcm(N, P, 6300)
    recv = T.bernoulli_recv(N, P, 0.2, 29)
    b = solo_amd.SoloBatch(N, encoder=True, decoder=True, slot_bytes=512)
    enc_only, dec_only = [1, 5, 9, 13], [2, 6, 10, 14]
    h1 = _run(torch_cuda, b, pcm[:, :H], recv[:, :H])
    b.reset_streams(enc_only, rate=[15600, 24000, 15600, 24000], which="enc")   # (useMDIndex unchanged: the old decoder reads the new bits)
    b.reset_streams(dec_only, which="dec")
    h2 = _run(torch_cuda, b, pcm[:, H:], recv[:, H:])
    hb, hn, ho = (np.concatenate([x, y], axis=1) for x, y in zip(h1, h2))
    for i in range(N):
        e, d = R.RefEncoder("fix"), R.RefDecoder("fix")
        for p in range(P):
            if p == H and i in enc_only:
                e = R.RefEncoder("fix", rate=[15600, 24000, 15600, 24000][enc_only.index(i)])
            if p == H and i in dec_only:
                d = R.RefDecoder("fix")
            pl, n0, n1 = e.encode(pcm[i, p])
            _check_enc(hb, hn, i, p, (pl, n0, n1))
            y, ret = d.decode(*_ref_call(pl, n0, n1, int(recv[i, p])))
            assert ret == 0 and np.array_equal(ho[i, p], y), (i, p)


def test_reset_of_every_stream_equals_batch_reset(torch_cuda):
    import solo_amd
    N, P = 16, 6
    pcm = _pcm(N, 2 * P, 7400)
    recv = T.bernoulli_recv(N, 2 * P, 0.3, 31)
    outs = []
    for full in (True, False):
        b = solo_amd.SoloBatch(N, encoder=True, decoder=True, slot_bytes=512, use_md_index=1, dtx=1)
        _run(torch_cuda, b, pcm[:, :P], recv[:, :P])
        if full:
            b.reset()
        else:
            assert b.lib.solo_batch_reset_streams(b.h, (C.c_int32 * N)(*range(N)), N, 3, None, None, b._stream()) == 0
        outs.append(_run(torch_cuda, b, pcm[:, P:], recv[:, P:]))
    for x, y in zip(*outs):
        assert np.array_equal(x, y)


@need_ref
@pytest.mark.parametrize("mode", ["32k", "20ms"])
def test_other_modes_mixed(torch_cuda, mode):
    import solo_amd
    N, P = 64, 8
    if mode == "32k":
        kw = dict(samplerate=32000)
        ctl = [((15600, 24000)[i % 2], 0, (i // 2) % 2) for i in range(N)]
        pcm = _pcm(N, P, 8100, quiet=[(3, 7)], samples=1280)
        b = solo_amd.SoloBatch(N, rate=15600, encoder=True, decoder=True, slot_bytes=512, samplerate=32000)
    else:
        kw = dict(framesize_ms=20)
        ctl = [COMBOS[(i * 5) % len(COMBOS)] for i in range(N)]
        pcm = _pcm(N, P, 8200, quiet=[(2, 7)], samples=320)
        b = solo_amd.SoloBatch(N, encoder=True, decoder=True, slot_bytes=512, framesize_ms=20)
    recv = T.bernoulli_recv(N, P, 0.3, 37)
    b.reset_streams(range(N), rate=[c[0] for c in ctl], dtx=[c[1] for c in ctl], use_md_index=[c[2] for c in ctl])
    hb, hn, ho = _run(torch_cuda, b, pcm, recv)
    refs = {i: _Ref(*ctl[i], **kw) for i in range(N)}
    _check_streams(hb, hn, ho, recv, pcm, refs, range(N))


def _enc_ctrls(n, **over):
    import solo_amd
    arr = (solo_amd.USER_Ctrl_enc * n)()
    for i in range(n):
        c = solo_amd.default_enc_ctrl()
        for k, v in over.items():
            setattr(c, k, v)
        arr[i] = c
    return arr


def _dec_ctrls(n, **over):
    import solo_amd
    arr = (solo_amd.USER_Ctrl_dec * n)()
    for i in range(n):
        c = solo_amd.default_dec_ctrl()
        for k, v in over.items():
            setattr(c, k, v)
        arr[i] = c
    return arr


@need_ref
def test_refused_calls_change_nothing(torch_cuda):
    import solo_amd
    torch = torch_cuda
    N, P, H = 8, 6, 3
    pcm = _pcm(N, P, 9100)
    recv = T.bernoulli_recv(N, P, 0.2, 41)
    b = solo_amd.SoloBatch(N, encoder=True, decoder=True, slot_bytes=512)
    lib, st = b.lib, b._stream()
    ix = lambda *v: (C.c_int32 * len(v))(*v)
    h1 = _run(torch, b, pcm[:, :H], recv[:, :H])
    refused = [
        (ix(0, N), 2, 3, None, None),                                   # index out of range
        (ix(-1), 1, 3, None, None),
        (ix(1, 1), 2, 3, None, None),                                   # listed twice
        (ix(0), 0, 3, None, None),                                      # n <= 0
        (ix(*range(N)), N + 1, 3, None, None),                          # n > N
        (ix(0), 1, 0, None, None),                                      # which
        (ix(0), 1, 1, _enc_ctrls(1, samplerate=32000, targetRate_bps=24000), None),
        (ix(0), 1, 1, _enc_ctrls(1, framesize_ms=20), None),
        (ix(0), 1, 1, _enc_ctrls(1, joint_enable=1, joint_mode=1), None),
        (ix(0), 1, 2, None, _dec_ctrls(1, samplerate=32000)),
        (ix(0), 1, 2, None, _dec_ctrls(1, framesize_ms=20)),
        (ix(0), 1, 2, None, _dec_ctrls(1, joint_enable=1, joint_mode=1)),
        (ix(0), 1, 2, _enc_ctrls(1), None),                             # an encoder control in a decoder-only call
        (ix(0, 3), 2, 3, _enc_ctrls(2, useMDIndex=1), _dec_ctrls(2, framesize_ms=20)),   # one bad control refuses the whole call
    ]
    for args in refused:
        assert lib.solo_batch_reset_streams(b.h, args[0], args[1], args[2], args[3], args[4], st) == -1, args[1:3]
    for bad in (dict(streams=[0, N]), dict(streams=[2, 2]), dict(streams=[])):
        with pytest.raises(ValueError):
            b.reset_streams(**bad)
    h2 = _run(torch, b, pcm[:, H:], recv[:, H:])
    hb, hn, ho = (np.concatenate([x, y], axis=1) for x, y in zip(h1, h2))
    _check_streams(hb, hn, ho, recv, pcm, {i: _Ref() for i in range(N)}, range(N))

    # 32 kHz: a 13600 bps stream would leave SILK below 14 kbps (not built) -- refused, the handle goes on unchanged
    P32 = 4
    x32 = _pcm(2, P32, 9200, samples=1280)
    r32 = np.full((2, P32), 3, np.uint8)
    w = solo_amd.SoloBatch(2, rate=15600, encoder=True, decoder=True, slot_bytes=512, samplerate=32000)
    g1 = _run(torch, w, x32[:, :2], r32[:, :2])
    assert w.lib.solo_batch_reset_streams(w.h, ix(1), 1, 1, _enc_ctrls(1, samplerate=32000, targetRate_bps=13600), None, w._stream()) == -1
    with pytest.raises(ValueError):
        w.reset_streams([1], rate=13600)
    g2 = _run(torch, w, x32[:, 2:], r32[:, 2:])
    hb, hn, ho = (np.concatenate([x, y], axis=1) for x, y in zip(g1, g2))
    _check_streams(hb, hn, ho, r32, x32, {i: _Ref(15600, samplerate=32000) for i in range(2)}, range(2))

    # decoder-only handle: an encoder control (or the encoder direction) is refused
    d = solo_amd.SoloBatch(2, encoder=False, decoder=True, slot_bytes=512)
    assert d.lib.solo_batch_reset_streams(d.h, ix(0), 1, 3, _enc_ctrls(1), None, d._stream()) == -1
    assert d.lib.solo_batch_reset_streams(d.h, ix(0), 1, 1, None, None, d._stream()) == -1
    assert d.lib.solo_batch_reset_streams(d.h, ix(0), 1, 2, _enc_ctrls(1), None, d._stream()) == -1
    with pytest.raises(ValueError):
        d.reset_streams([0], rate=24000)
    refs = [_Ref() for _ in range(2)]
    payload = [[refs[i].e.encode(pcm[i, p]) for p in range(P)] for i in range(2)]
    bits, nb = T.pack_slots(payload, 512)
    out, _ = d.decode(torch.from_numpy(bits).to(d.device), torch.from_numpy(nb).to(d.device), None)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    for i in range(2):
        for p in range(P):
            y, ret = refs[i].d.decode(*payload[i][p], 4)
            assert ret == 0 and np.array_equal(out[i, p], y), (i, p)


def _arrivals(streams, seq0, payload, desc_known):
    """all descriptions of payload[i][p] as arrivals for seq0[i] + p: int32 [n, 5] + the byte pool"""
    rows, pool = [], bytearray()
    for i in streams:
        for p, (pl, n0, n1) in enumerate(payload[i]):
            for dsc, part in ((0, pl[:n0 - n1]), (1, pl[n0 - n1:n0])):
                rows.append((i, seq0[i] + p, dsc if desc_known else -1, len(pool), len(part)))
                pool += part
    return np.array(rows, np.int32), np.frombuffer(bytes(pool), np.uint8).copy()


@need_ref
def test_receiver_ring_per_stream_index_and_stream_reset(torch_cuda):
    import solo_amd
    torch = torch_cuda
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    # (a) useMDIndex alternating over the streams: desc = -1 is filed for the useMDIndex = 1 streams, counted bad for the others
    N, P = 8, 6
    pcm = _pcm(N, P, 9400)
    b = solo_amd.SoloBatch(N, encoder=False, decoder=True, slot_bytes=512)
    mds = [i % 2 for i in range(N)]
    b.reset_streams(range(N), use_md_index=mds)
    refs = [_Ref(md=mds[i]) for i in range(N)]
    payload = [[refs[i].e.encode(pcm[i, p]) for p in range(P)] for i in range(N)]
    b.recv_create(8, 256, 0)
    arr, pool = _arrivals(range(N), [0] * N, payload, desc_known=False)
    b.recv_insert(dev(arr), dev(pool))
    st = b.recv_stats()
    assert st["inserted"] == 2 * P * sum(mds) and st["bad"] == 2 * P * (N - sum(mds)), st
    out, status = b.recv_decode(P)
    out = out.cpu().numpy()
    for i in range(N):
        if mds[i]:
            for p in range(P):
                y, ret = refs[i].d.decode(*payload[i][p], 4)
                assert ret == 0 and np.array_equal(out[i, p], y), (i, p)

    # (b) recv_reset_streams on a subset mid-way through play-out, with the decoder state reset as a joining call would
    N, P, D = 8, 12, 16
    pcm = _pcm(N, P, 9500)
    b = solo_amd.SoloBatch(N, encoder=False, decoder=True, slot_bytes=512, use_md_index=1)
    refs = [_Ref(md=1) for _ in range(N)]
    payload = [[refs[i].e.encode(pcm[i, p]) for p in range(P)] for i in range(N)]
    b.recv_create(D, 256, 0)
    arr, pool = _arrivals(range(N), [0] * N, payload, desc_known=True)
    b.recv_insert(dev(arr), dev(pool))
    out1, _ = b.recv_decode(4)
    subset, first = [1, 4, 6], [100, 100, 37]
    b.reset_streams(subset)
    b.recv_reset_streams(subset, first)
    fresh = {i: _Ref(md=1) for i in subset}
    pcm2 = _pcm(N, 6, 9600)
    pay2 = {i: [fresh[i].e.encode(pcm2[i, p]) for p in range(6)] for i in subset}
    arr2, pool2 = _arrivals(subset, dict(zip(subset, first)), pay2, desc_known=False)
    b.recv_insert(dev(arr2), dev(pool2))
    st = b.recv_stats()
    assert st["inserted"] == 2 * P * N + 2 * 6 * len(subset) and st["duplicate"] == 0, st     # statistics carried on; queues emptied
    out2, _ = b.recv_decode(6)
    torch.cuda.synchronize()
    out = np.concatenate([out1.cpu().numpy(), out2.cpu().numpy()], axis=1)
    for i in range(N):
        for p in range(10):
            if i in subset and p >= 4:
                y, ret = fresh[i].d.decode(*pay2[i][p - 4], 4)
            else:
                y, ret = refs[i].d.decode(*payload[i][p], 4)
            assert ret == 0 and np.array_equal(out[i, p], y), (i, p)

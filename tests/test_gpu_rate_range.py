"""The whole targetRate_bps range on the GPU, against the compiled reference.  The encoder clamps the SILK rate (target rate minus the
high-band share) to [5000, 100000] (enc_API.c:187) and maps it to an SNR through the 8-knot tables of SKP_Silk_setup_rate_FIX, once for
the whole rate (`<=`) and once per description at half the rate (`<`).  The other GPU tests run a handful of rates between 13600 and
40000 bps; here every clamp and every knot of both modes, on full-scale edge signals as well as speech, where the quantiser's pulses grow
large and packets outgrow what the decoder stages in LDS (252 B) -- the quantiser rows, the range coder, the extraction records and the
single-kernel decoder's HBM branch all meet inputs that the narrow band never gives them.  Every stream is compared with a reference
encoder / decoder created with that stream's own control: payloads and lengths byte-exact, PCM sample-exact."""
import ctypes as C

import numpy as np
import pytest

import refcodec as R
import solo_testlib as T
from solo_amd.synth import EDGE_FAMILIES, edge_stream

pytestmark = pytest.mark.gpu
need_ref = pytest.mark.skipif(not R.have_ref("fix"), reason="oracle/_ref not present on this box")

I32_MAX = 2 ** 31 - 1
HB_BPS = 1600                                           # the high-band share of the target rate (AGR_BWE_SDK_API.c:119); 800 with joint
KNOTS_NB = (8000, 9000, 11000, 13000, 16000, 22000)     # TargetRate_table_NB[1..6] (SKP_Silk_tables_other.c)
KNOTS_WB = (11000, 14000, 17000, 21000, 26000, 36000)   # TargetRate_table_WB[1..6]
LDS_BYTES = 252                                         # larger packets are read from HBM by the decoder, refused by the receiver front end


def _uniq(v):
    return list(dict.fromkeys(v))


# 16 kHz: <= 0 means 15600; SILK rates <= 5000 clamp up (1, 1600, 6599, 6600), > 100000 down; every knot k as SILK rate k / k + 1 (the
# whole-rate table) and 2k / 2k + 1 (the per-description table at half the rate)
RATES_16 = _uniq([0, -1, 1, 1600, 6599, 6600, 6601] + [HB_BPS + m * k + d for k in KNOTS_NB for m in (1, 2) for d in (0, 1)]
                 + [101600, 101601, 150000, I32_MAX])
# 32 kHz: SILK >= 14000 (15600 without joint, 14800 with it); knots below that are reached only as 2k
RATES_32 = _uniq([15600, 15601] + [HB_BPS + m * k for k in KNOTS_WB for m in (1, 2) if m * k >= 14000] + [101600, 150000, I32_MAX])
RATES_32_JOINT = [14800, 14801, 22800, 101600, I32_MAX]
N_SPEECH = 3
P = 12
QUIET = (4, 10)                                          # packets of near-silence in the speech-like streams: DTX fires there


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch


def _signal(fam, n_packets, samples, seed0):
    """family < EDGE_FAMILIES: that edge family (read at the mode's sample rate); otherwise a speech-like stream with a quiet stretch"""
    n = n_packets * samples
    if fam < EDGE_FAMILIES:
        x = edge_stream(seed0 * EDGE_FAMILIES + fam, -(-n // 640)).reshape(-1)[:n]
    else:
        x = R.synth_stream(seed0 + fam, -(-n // 640)).reshape(-1)[:n].copy()
        rng = np.random.default_rng(seed0 + fam)
        a, e = min(QUIET[0] * samples, n), min(QUIET[1] * samples, n)
        x[a:e] = (rng.standard_normal(e - a) * 3).astype(np.int16)
    return np.ascontiguousarray(x.reshape(n_packets, samples))


def _ref_call(pl, n0, n1, m):
    """the decoder call the batched API makes of one record: an empty (DTX) record is concealed as lost"""
    if n0 == 0:
        return b"", 16, 0, 1
    return R.map_loss(pl, n0, n1, not (m & 1), not (m & 2))


class Matrix:
    """rates x signals in one handle: stream i has rate rates[i // S] and signal fams[i % S]; DTX and useMDIndex follow the signal, so
    that streams of one signal differ in their rate alone"""

    def __init__(self, rates, fams, samples, seed0, joint=0, **kw):
        self.rates, self.fams, self.kw, self.joint = rates, fams, kw, joint
        S = len(fams)
        self.N = len(rates) * S
        self.rate = [rates[i // S] for i in range(self.N)]
        self.sig = [i % S for i in range(self.N)]
        self.dtx = [(s + 1) % 2 for s in self.sig]
        self.md = [(s // 2) % 2 for s in self.sig]
        sigs = [_signal(f, P, samples, seed0) for f in fams]
        self.pcm = np.stack([sigs[s] for s in self.sig])
        self.masks = {"all": np.full((self.N, P), 3, np.uint8), "loss": T.bernoulli_recv(self.N, P, 0.3, seed0)}
        self._ref = None

    def ref(self):
        """the reference's payloads [N][P] of (bytes, n0, n1) and its PCM under each mask"""
        if self._ref is None:
            enc, pcm = [], {k: np.zeros(self.pcm.shape, np.int16) for k in self.masks}
            for i in range(self.N):
                e = R.RefEncoder("fix", rate=self.rate[i], dtx=self.dtx[i], use_md_index=self.md[i], joint=self.joint, **self.kw)
                enc.append([e.encode(self.pcm[i, p]) for p in range(P)])
                for k, m in self.masks.items():
                    d = R.RefDecoder("fix", use_md_index=self.md[i], joint=self.joint, **self.kw)
                    for p, (pl, n0, n1) in enumerate(enc[i]):
                        y, ret = d.decode(*_ref_call(pl, n0, n1, int(m[i, p])))
                        assert ret == 0
                        pcm[k][i, p] = y
            self._ref = enc, pcm
        return self._ref

    def check_encoded(self, hb, hn, streams=None):
        enc, _ = self.ref()
        for i in range(self.N) if streams is None else streams:
            for p in range(P):
                pl, n0, n1 = enc[i][p]
                assert (int(hn[i, p, 0]), int(hn[i, p, 1])) == (n0, n1), (self.rate[i], self.fams[self.sig[i]], p)
                assert hb[i, p, :n0].tobytes() == pl[:n0], (self.rate[i], self.fams[self.sig[i]], p)

    def streams_at(self, rate):
        return [i for i in range(self.N) if self.rate[i] == rate]


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _encode(torch, b, pcm):
    bits, nb, st = b.encode(_dev(torch, pcm))
    torch.cuda.synchronize()
    assert int(st.abs().max()) == 0
    return bits.cpu().numpy(), nb.cpu().numpy()


def _decode_all_masks(torch, mx, hb, hn, slot, **create):
    """a fresh decoder-only handle per mask (created after the test set its knobs), every stream reset to its own useMDIndex"""
    import solo_amd
    out = {}
    for k, m in mx.masks.items():
        d = solo_amd.SoloBatch(mx.N, encoder=False, decoder=True, slot_bytes=slot, **create)
        d.reset_streams(range(mx.N), use_md_index=mx.md)
        y, st = d.decode(_dev(torch, hb), _dev(torch, hn), _dev(torch, m))
        torch.cuda.synchronize()
        assert int(st.abs().max()) == 0, k
        out[k] = y.cpu().numpy()
        d.close()
    return out


def _check_decoded(mx, out):
    _, ref = mx.ref()
    for k in mx.masks:
        bad = np.nonzero((out[k] != ref[k]).any(axis=2))
        assert bad[0].size == 0, (k, "first differing (rate, family, packet)", mx.rate[int(bad[0][0])], mx.fams[mx.sig[int(bad[0][0])]], int(bad[1][0]))


def _same_bytes(hb, hn, a, b):
    return np.array_equal(hn[a], hn[b]) and all(hb[a, p, :hn[a, p, 0]].tobytes() == hb[b, p, :hn[b, p, 0]].tobytes() for p in range(hn.shape[1]))


def _assert_clamps(mx, hb, hn, groups):
    """streams whose rates clamp to the same SILK rate must give the same bytes on the same signal"""
    S = len(mx.fams)
    for g in groups:
        base = mx.streams_at(g[0])
        for r in g[1:]:
            for a, b in zip(base, mx.streams_at(r)):
                assert _same_bytes(hb, hn, a, b), (g[0], r, mx.fams[mx.sig[a]])
        assert S == len(base)


def _assert_coverage(mx, hn):
    dtx_streams = [i for i in range(mx.N) if mx.dtx[i]]
    assert int((hn[dtx_streams, :, 0] == 0).sum()) > 0                                     # DTX fired
    assert int((hn[[i for i in range(mx.N) if not mx.dtx[i]], :, 0] == 0).sum()) == 0
    assert int(hn[..., 0].max()) > LDS_BYTES                                               # the decoder's HBM branch is taken
    assert set(mx.md) == {0, 1}


# ---- (a) 16 kHz: every clamp and knot x every edge family + speech, in one handle ------------------------------------------------
_M16 = {}


def _m16(torch):
    """31 rates x 17 signals = 527 streams (not a multiple of 4 or 32: ragged quantiser rows and range-coder waves), encoded once"""
    if "enc" not in _M16:
        import solo_amd
        mx = Matrix(RATES_16, list(range(EDGE_FAMILIES + N_SPEECH)), 640, 1)
        b = solo_amd.SoloBatch(mx.N, encoder=True, decoder=False, slot_bytes=1024)
        b.reset_streams(range(mx.N), rate=mx.rate, dtx=mx.dtx, use_md_index=mx.md)
        _M16["mx"], _M16["enc"] = mx, _encode(torch, b, mx.pcm)
        b.close()
    return _M16["mx"], _M16["enc"]


# the decoder paths: the default two kernels, the single kernel (the one that reads payloads above 252 B from HBM), small chunks
DEC_PATHS = [{}, {"SOLO_DEC_SPLIT": "0"}, {"SOLO_DEC_CHUNK": "3", "SOLO_DEC_FIRST_CHUNK": "2"}]
_ids = lambda k: ",".join("%s=%s" % kv for kv in k.items()) or "default"


@need_ref
@pytest.mark.parametrize("knobs", DEC_PATHS, ids=_ids)
def test_rate_matrix_16k_vs_reference(torch_cuda, monkeypatch, knobs):
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)                                        # read at a handle's first decode
    mx, (hb, hn) = _m16(torch_cuda)
    assert mx.N % 2 == 1 and mx.N % 4 and mx.N % 32
    _assert_coverage(mx, hn)
    _assert_clamps(mx, hb, hn, [(0, -1), (6600, 1, 1600, 6599), (101600, 101601, 150000, I32_MAX)])
    mx.check_encoded(hb, hn)
    _check_decoded(mx, _decode_all_masks(torch_cuda, mx, hb, hn, 1024))


# ---- (b) the rate given at creation instead of per stream --------------------------------------------------------------------------
@need_ref
@pytest.mark.parametrize("rate", [0, 1, 6600, 101600, I32_MAX])
def test_create_time_rate_equals_per_stream_rate(torch_cuda, rate):
    import solo_amd
    mx, (hb, hn) = _m16(torch_cuda)
    for dtx in (0, 1):
        for md in (0, 1):
            idx = [i for i in mx.streams_at(rate) if mx.dtx[i] == dtx and mx.md[i] == md]
            assert idx
            b = solo_amd.SoloBatch(len(idx), rate=rate, encoder=True, decoder=False, slot_bytes=1024, dtx=dtx, use_md_index=md)
            gb, gn = _encode(torch_cuda, b, mx.pcm[idx])
            b.close()
            assert np.array_equal(gn, hn[idx]) and np.array_equal(gb, hb[idx]), (rate, dtx, md)
            enc, _ = mx.ref()
            for j, i in enumerate(idx):
                for p in range(P):
                    pl, n0, n1 = enc[i][p]
                    assert (int(gn[j, p, 0]), int(gn[j, p, 1])) == (n0, n1) and gb[j, p, :n0].tobytes() == pl[:n0], (rate, i, p)


# ---- (c) 32 kHz: the same over its range, refused rates included -------------------------------------------------------------------
def _enc_ctrl_arr(**kw):
    import solo_amd
    arr = (solo_amd.USER_Ctrl_enc * 1)()
    arr[0] = solo_amd.default_enc_ctrl(**kw)
    return arr


_M32 = {}


def _m32(torch, joint):
    """every edge family but 2 (the reference overflows its stack on full-scale square waves at 32 kHz: make_edge_golden.py) + two
    speech-like signals: 15 x 15 = 225 (joint: 5 x 15 = 75) streams.  The packets are encoded in two calls with refused resets in
    between, which must change nothing."""
    if joint not in _M32:
        import solo_amd
        fams = [f for f in range(EDGE_FAMILIES + 2) if f != 2]
        rates = RATES_32_JOINT if joint else RATES_32
        mx = Matrix(rates, fams, 1280, 2 + joint, joint=joint, samplerate=32000)
        b = solo_amd.SoloBatch(mx.N, rate=rates[0], encoder=True, decoder=False, slot_bytes=1024, samplerate=32000, joint=joint)
        b.reset_streams(range(mx.N), rate=mx.rate, dtx=mx.dtx, use_md_index=mx.md)
        H = P // 2
        hb1, hn1 = _encode(torch, b, mx.pcm[:, :H])
        low = 14799 if joint else 15599                                  # SILK 13999: the 32 kHz build has no tables below 14000
        with pytest.raises(ValueError):
            b.reset_streams([1], rate=low)
        with pytest.raises(ValueError):
            b.reset_streams(range(mx.N), rate=[rates[0]] * (mx.N - 1) + [low])
        ix = (C.c_int32 * 2)(0, 3)
        arr = (solo_amd.USER_Ctrl_enc * 2)(solo_amd.default_enc_ctrl(rates[0], joint=joint, samplerate=32000),
                                           solo_amd.default_enc_ctrl(low, joint=joint, samplerate=32000))
        assert b.lib.solo_batch_reset_streams(b.h, ix, 2, 1, arr, None, b._stream()) == -1
        hb2, hn2 = _encode(torch, b, mx.pcm[:, H:])
        b.close()
        _M32[joint] = mx, (np.concatenate([hb1, hb2], axis=1), np.concatenate([hn1, hn2], axis=1))
    return _M32[joint]


@pytest.mark.parametrize("joint", [0, 1])
def test_32k_rates_below_silk_14000_are_refused(torch_cuda, joint):
    import solo_amd
    low = 14799 if joint else 15599
    with pytest.raises(RuntimeError):
        solo_amd.SoloBatch(3, rate=low, encoder=True, decoder=False, samplerate=32000, joint=joint)
    solo_amd.SoloBatch(3, rate=low + 1, encoder=True, decoder=False, samplerate=32000, joint=joint).close()
    lib = solo_amd.load_library()
    c = solo_amd.default_enc_ctrl(low, joint=joint, samplerate=32000)
    assert not lib.AGR_Sate_Encoder_Init(C.byref(c))


@need_ref
@pytest.mark.parametrize("joint", [0, 1], ids=["plain", "joint"])
@pytest.mark.parametrize("knobs", DEC_PATHS, ids=_ids)
def test_rate_matrix_32k_vs_reference(torch_cuda, monkeypatch, knobs, joint):
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    mx, (hb, hn) = _m32(torch_cuda, joint)
    assert mx.N % 2 == 1 and mx.N % 4 and mx.N % 32
    _assert_coverage(mx, hn)
    _assert_clamps(mx, hb, hn, [tuple(r for r in (101600, 150000, I32_MAX) if r in mx.rates)])
    mx.check_encoded(hb, hn)
    _check_decoded(mx, _decode_all_masks(torch_cuda, mx, hb, hn, 1024, samplerate=32000, joint=joint))


# ---- (d) framesize 20 at the extremes (this mode always runs the single-kernel decoder) ---------------------------------------------
@need_ref
@pytest.mark.parametrize("fs", [16000, 32000])
def test_framesize20_at_the_extremes_vs_reference(torch_cuda, fs):
    import solo_amd
    if fs == 16000:
        rates, fams = [1, 6600, HB_BPS + 13000, HB_BPS + 2 * 16000, 101600, I32_MAX], list(range(EDGE_FAMILIES + N_SPEECH))
    else:
        rates, fams = [15600, HB_BPS + 2 * 21000, 101600, I32_MAX], [f for f in range(EDGE_FAMILIES + N_SPEECH) if f != 2]
    mx = Matrix(rates, fams, 320 * fs // 16000, 4, samplerate=fs, framesize_ms=20)
    b = solo_amd.SoloBatch(mx.N, rate=rates[0], encoder=True, decoder=False, slot_bytes=1024, samplerate=fs, framesize_ms=20)
    b.reset_streams(range(mx.N), rate=mx.rate, dtx=mx.dtx, use_md_index=mx.md)
    hb, hn = _encode(torch_cuda, b, mx.pcm)
    assert int((hn[[i for i in range(mx.N) if mx.dtx[i]], :, 0] == 0).sum()) > 0
    _assert_clamps(mx, hb, hn, [(101600, I32_MAX)])
    mx.check_encoded(hb, hn)
    _check_decoded(mx, _decode_all_masks(torch_cuda, mx, hb, hn, 1024, samplerate=fs, framesize_ms=20))


# ---- (e) the receiver front end at its size limit ----------------------------------------------------------------------------------
SMALL = [(r, f) for r in (6600, 15600, 24000) for f in (0, 1, 3, 4, 5, 6, 7, 8, 10, 11, 12, 13, EDGE_FAMILIES)]
LARGE = [(I32_MAX, f) for f in (1, 2, 6, 9)]


@need_ref
def test_receiver_front_end_at_its_size_limit(torch_cuda):
    """Packets up to 252 B are decoded exactly by solo_batch_decode_split and by the staging ring; a stream whose packets grow beyond that
    reports -11 in both (pinned: the front end stages a packet in LDS), while the other streams of the same call stay exact."""
    import solo_amd
    torch = torch_cuda
    ctl = [SMALL[i // 2] if i % 2 == 0 or i // 2 >= len(LARGE) else LARGE[i // 2] for i in range(len(SMALL) + len(LARGE))]
    N, SL = len(ctl), 512
    big = [i for i in range(N) if ctl[i] in LARGE]
    assert len(big) == len(LARGE)
    pcm = np.stack([_signal(f, P, 640, 5) for _, f in ctl])
    payload = []
    for i in range(N):
        e = R.RefEncoder("fix", rate=ctl[i][0])
        payload.append([e.encode(pcm[i, p]) for p in range(P)])
    n0 = np.array([[n for _, n, _ in payload[i]] for i in range(N)])
    assert (n0[big] > LDS_BYTES).any(axis=1).all() and (n0[[i for i in range(N) if i not in big]] <= LDS_BYTES).all()
    assert (n0 > 0).all()

    def want(i, recv):
        d = R.RefDecoder("fix")
        out = []
        for p, (pl, a, b) in enumerate(payload[i]):
            y, ret = d.decode(*_ref_call(pl, a, b, int(recv[i, p])))
            assert ret == 0
            out.append(y)
        return np.stack(out)

    # (1) one decode_split call: descriptions in their arrival slots, 30 % of them lost
    recv = T.bernoulli_recv(N, P, 0.3, 43)
    dA, dB = np.zeros((N, P, SL), np.uint8), np.zeros((N, P, SL), np.uint8)
    lA, lB = np.zeros((N, P), np.int16), np.zeros((N, P), np.int16)
    for i in range(N):
        for p, (pl, a, b) in enumerate(payload[i]):
            x = np.frombuffer(pl, np.uint8)
            if recv[i, p] & 1:
                dA[i, p, :a - b] = x[:a - b]; lA[i, p] = a - b
            if recv[i, p] & 2:
                dB[i, p, :b] = x[a - b:a]; lB[i, p] = b
    assert all((lA[i].astype(int) + lB[i] > LDS_BYTES).any() for i in big)
    h = solo_amd.SoloBatch(N, encoder=False, decoder=True, slot_bytes=SL)
    y, st = h.decode_split(_dev(torch, dA), _dev(torch, lA), _dev(torch, dB), _dev(torch, lB))
    torch.cuda.synchronize()
    y, st = y.cpu().numpy(), st.cpu().numpy()
    for i in range(N):
        if i in big:
            assert st[i] == -11, (i, ctl[i])
        else:
            assert st[i] == 0 and np.array_equal(y[i], want(i, recv)), (i, ctl[i])

    # (2) one play-out of the staging ring: every description arrives, in one insert
    rows, pool = [], bytearray()
    for i in range(N):
        for p, (pl, a, b) in enumerate(payload[i]):
            for dsc, part in ((0, pl[:a - b]), (1, pl[a - b:a])):
                rows.append((i, p, dsc, len(pool), len(part)))
                pool += part
    r = solo_amd.SoloBatch(N, encoder=False, decoder=True, slot_bytes=SL)
    r.recv_create(P, SL, 0)
    r.recv_insert(_dev(torch, np.array(rows, np.int32)), _dev(torch, np.frombuffer(bytes(pool), np.uint8).copy()))
    stats = r.recv_stats()
    assert stats["inserted"] == 2 * N * P and stats["bad"] == 0, stats
    y, st = r.recv_decode(P)
    torch.cuda.synchronize()
    y, st = y.cpu().numpy(), st.cpu().numpy()
    every = np.full((N, P), 3, np.uint8)
    for i in range(N):
        if i in big:
            assert st[i] == -11, (i, ctl[i])
        else:
            assert st[i] == 0 and np.array_equal(y[i], want(i, every)), (i, ctl[i])


# ---- (f) the legacy symbols at the top rate ----------------------------------------------------------------------------------------
@need_ref
@pytest.mark.parametrize("fs,rate", [(16000, 101600), (32000, I32_MAX)])
def test_legacy_api_at_the_top_rate_vs_reference(torch_cuda, fs, rate):
    """AGR_Sate_Encoder_Encode / AGR_Sate_Decoder_Decode one packet at a time, with what both libraries leave in the caller's nBytes
    arrays, on packets far larger than the batched path's default slot (up to ~600 B)"""
    import solo_amd
    lib = solo_amd.load_library()
    ns = 640 * fs // 16000
    x = np.concatenate([_signal(f, 8, ns, 6) for f in (9, 1, 6, EDGE_FAMILIES)])
    ctrl = solo_amd.default_enc_ctrl(rate, samplerate=fs)
    h = lib.AGR_Sate_Encoder_Init(C.byref(ctrl))
    assert h
    er = R.RefEncoder("fix", rate=rate, samplerate=fs)
    buf = np.zeros(1024, np.uint8)
    recs = []
    for p in range(x.shape[0]):
        xp = np.ascontiguousarray(x[p])
        nbv = np.full(6, 77, np.int16)
        n = lib.AGR_Sate_Encoder_Encode(h, xp.ctypes.data, buf.ctypes.data, 1024, nbv.ctypes.data)
        er._nb[:] = 77
        nr = er.lib.AGR_Sate_Encoder_Encode(er.h, xp.ctypes.data, er._bits.ctypes.data, 1024, er._nb.ctypes.data)
        assert n == nr and np.array_equal(nbv, er._nb), (p, n, nr, nbv, er._nb)
        assert buf[:n].tobytes() == er._bits[:n].tobytes(), p
        recs.append((buf[:n].tobytes(), int(nbv[0]), int(nbv[1])))
    lib.AGR_Sate_Encoder_Uninit(h)
    assert max(n0 for _, n0, _ in recs) > (500 if fs == 32000 else 300)
    dctrl = solo_amd.default_dec_ctrl(samplerate=fs)
    hd = lib.AGR_Sate_Decoder_Init(C.byref(dctrl))
    dr = R.RefDecoder("fix", samplerate=fs)
    pat = R.cli_loss_pattern(len(recs), 30)
    out = np.zeros(1920, np.int16)
    ns_out = np.zeros(1, np.int16)
    flags = set()
    for p, (pl, n0, n1) in enumerate(recs):
        pay, a0, a1, flag = R.map_loss(pl, n0, n1, *pat[p])
        flags.add(flag)
        b = np.zeros(1100, np.uint8)
        b[:len(pay)] = np.frombuffer(pay, np.uint8)
        nbv = np.array([a0, a1, 55, 55, 55, 55], np.int16)
        ns_out[0] = -1
        ret = lib.AGR_Sate_Decoder_Decode(hd, out.ctypes.data, ns_out.ctypes.data, b.ctypes.data, nbv.ctypes.data, flag)
        y, r1 = dr.decode(pay, a0, a1, flag)
        assert ret == r1 == 0 and np.array_equal(out[:ns], y), (p, flag)
        assert (int(nbv[0]), int(nbv[1])) == dr.nbytes_after, (p, flag, nbv[:2], dr.nbytes_after)
        assert list(nbv[2:]) == [55] * 4 and int(ns_out[0]) == dr.nsamples_out == ns
    assert flags == {1, 2, 3, 4}
    lib.AGR_Sate_Decoder_Uninit(hd)

"""Call-length parity on the GPU: the 1250-packet streams of tests/golden/long_horizon.npz (the compiled reference's answers, see
tests/test_long_horizon.py for what changes that late in a call) through the C ABI, bit-exact: lengths and payload CRC of every packet,
PCM CRC of every decoded packet under the clean decode and the three arrival masks (30 % loss, a call on hold, minutes on one
description); empty DTX records are lost packets.

  call shapes      one call of 1250 packets, 25 state-continued calls of 50, and for two rows 1250 calls of one packet
  many copies      the 16 kHz rows tiled over 71 streams (18 waves of the four-streams-per-wave quantiser, the last one ragged)
  variants         SOLO_ENC_PERSIST=1, SOLO_ENC_CHUNK=0, SOLO_DEC_SPLIT=0
  stream control   resets at packets 300 and 700 (the VAD counter restarts), a rate change at 600 (it does not)
  receiver ring    every row: descriptions arrive separately and out of order at depth 8 and 3, through the hold and the DTX gaps; late ones are late
  fresh seeds      where oracle/_ref is present: against the compiled reference itself

Every case creates its handles once and stops at its first failure.  About 0.35 million packets each way in all."""
import zlib

import numpy as np
import pytest

import refcodec as R
import solo_testlib as T
import test_long_horizon as L
from recv_report_model import RingModel

pytestmark = pytest.mark.gpu
P = L.P
G16, J16, F16, W40, W20 = (0, 1, 2, 3, 5), (4,), (6,), (7, 8), (9,)       # fixture rows that can share a handle (fs, frame size, joint)
GROUPS = {"16k40": G16, "16k40joint": J16, "16k20": F16, "32k40": W40, "32k20": W20}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch


@pytest.fixture(scope="module")
def fx():
    return L.load_fixture()


_inputs = {}


def _input(fx, s):
    if s not in _inputs:
        _inputs[s] = L.stream_input(fx["cfg"][s], fx["quiet"])
    return _inputs[s]


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _crc_rows(a, lens=None):
    """CRC-32 of every [i, p] row of a (of its first lens[i, p] bytes)"""
    n, p = a.shape[:2]
    out = np.zeros((n, p), np.uint32)
    for i in range(n):
        for k in range(p):
            out[i, k] = zlib.crc32(a[i, k].tobytes() if lens is None else a[i, k, :lens[i, k]].tobytes())
    return out


def _first(bad):
    i, p = np.argwhere(bad)[0]
    return int(i), int(p)


class Handle:
    """one SoloBatch whose stream i is fixture row rows[i] (its own rate, DTX and useMDIndex) decoded under mask masks[i] (0 = clean)"""

    def __init__(self, torch, fx, rows, masks):
        import solo_amd
        self.torch, self.fx, self.rows, self.masks = torch, fx, list(rows), list(masks)
        cfg = fx["cfg"]
        r0 = cfg[self.rows[0]]
        assert all(tuple(cfg[s][[0, 1, 4]]) == tuple(r0[[0, 1, 4]]) for s in self.rows)
        self.ms = int(r0[1])
        self.b = solo_amd.SoloBatch(len(self.rows), rate=int(r0[2]), encoder=True, decoder=True, slot_bytes=512, use_md_index=int(r0[3]),
                                    joint=int(r0[4]), dtx=int(r0[5]), samplerate=int(r0[0]), framesize_ms=self.ms)
        assert self.b.packet_samples == L.packet_samples(int(r0[0]), self.ms)
        if any(tuple(cfg[s][[2, 3, 5]]) != tuple(r0[[2, 3, 5]]) for s in self.rows):
            self.b.reset_streams(list(range(len(self.rows))), rate=[int(cfg[s][2]) for s in self.rows], dtx=[int(cfg[s][5]) for s in self.rows],
                                 use_md_index=[int(cfg[s][3]) for s in self.rows], which="both")
        self.pcm = _dev(np.stack([_input(fx, s) for s in self.rows]))

    def encode(self, calls):
        torch, b = self.torch, self.b
        assert sum(calls) == P
        bits = torch.zeros((len(self.rows), P, 512), dtype=torch.uint8, device="cuda")
        nb = torch.zeros((len(self.rows), P, 2), dtype=torch.int16, device="cuda")
        a = 0
        worst = torch.zeros((), dtype=torch.int32, device="cuda")        # largest |status| of any call, kept on the device
        for c in calls:
            ob, on, st = b.encode(self.pcm[:, a:a + c].contiguous())
            bits[:, a:a + c], nb[:, a:a + c] = ob, on
            worst = torch.maximum(worst, st.abs().max())
            a += c
            if len(calls) <= 25:
                torch.cuda.synchronize()
                assert int(worst) == 0, "encode status, call ending at packet %d" % a
        torch.cuda.synchronize()
        assert int(worst) == 0, "encode status of one of %d calls" % len(calls)
        self.bits, self.nb = bits, nb
        self.hb, self.hn = bits.cpu().numpy(), nb.cpu().numpy()
        return self

    def check_encode(self, what=""):
        fx = self.fx
        want_n = fx["nbytes"][self.rows]
        if not np.array_equal(self.hn, want_n):
            i, p = _first((self.hn != want_n).any(axis=2))
            raise AssertionError("%s lengths: stream %d %s: %s, reference %s" % (what, i, L.where(self.rows[i], p, self.ms), self.hn[i, p].tolist(), want_n[i, p].tolist()))
        crc = _crc_rows(self.hb, self.hn[:, :, 0])
        want = fx["pcrc"][self.rows]
        if not np.array_equal(crc, want):
            i, p = _first(crc != want)
            raise AssertionError("%s payload: stream %d %s" % (what, i, L.where(self.rows[i], p, self.ms)))
        return self

    def recv(self):
        fx = self.fx
        m = np.stack([np.full(P, 3, np.uint8) if k == 0 else fx["masks"][k - 1, s] for s, k in zip(self.rows, self.masks)])
        m = m.copy()
        m[self.hn[:, :, 0] <= 0] = 0                               # an empty (DTX) record is a lost packet
        return m

    def decode(self, calls):
        torch, b = self.torch, self.b
        recv = _dev(self.recv())
        out = torch.zeros((len(self.rows), P, b.packet_samples), dtype=torch.int16, device="cuda")
        a = 0
        worst = torch.zeros((), dtype=torch.int32, device="cuda")
        for c in calls:
            y, st = b.decode(self.bits[:, a:a + c].contiguous(), self.nb[:, a:a + c].contiguous(), recv[:, a:a + c].contiguous())
            out[:, a:a + c] = y
            worst = torch.maximum(worst, st.abs().max())
            a += c
            if len(calls) <= 25:
                torch.cuda.synchronize()
                assert int(worst) == 0, "decode status, call ending at packet %d" % a
        torch.cuda.synchronize()
        assert int(worst) == 0, "decode status of one of %d calls" % len(calls)
        self.out = out.cpu().numpy()
        return self

    def check_decode(self, what=""):
        crc = _crc_rows(self.out)
        want = np.stack([self.fx["dcrc"][k, s] for s, k in zip(self.rows, self.masks)])
        if not np.array_equal(crc, want):
            i, p = _first(crc != want)
            raise AssertionError("%s PCM: stream %d, mask %s %s" % (what, i, L.MASK_NAMES[self.masks[i]], L.where(self.rows[i], p, self.ms)))
        return self

    def round_trip(self, calls, what=""):
        try:
            self.encode(calls).check_encode(what)
            self.decode(calls).check_decode(what)
        finally:
            self.b.close()


def _rows_x_masks(rows):
    return [s for s in rows for _ in range(4)], [k for _ in rows for k in range(4)]


@pytest.mark.parametrize("shape", ["1x1250", "25x50"])
@pytest.mark.parametrize("group", list(GROUPS))
def test_call_shapes(torch_cuda, fx, group, shape):
    rows, masks = _rows_x_masks(GROUPS[group])
    Handle(torch_cuda, fx, rows, masks).round_trip([P] if shape == "1x1250" else [50] * 25, "%s %s" % (group, shape))


@pytest.mark.parametrize("row", [0, 7])
def test_one_packet_per_call(torch_cuda, fx, row):
    rows, masks = _rows_x_masks((row,))
    Handle(torch_cuda, fx, rows, masks).round_trip([1] * P, "row %d, 1250 calls of one packet" % row)


def test_many_copies_at_once(torch_cuda, fx):
    """71 streams: 17 full waves of the quantiser's four streams and one with three; every lane position carries every row"""
    N = 71
    rows = [G16[i % len(G16)] for i in range(N)]
    masks = [(i // len(G16)) % 4 for i in range(N)]
    assert N % 4 and {(i % 4, r) for i, r in enumerate(rows)} == {(l, r) for l in range(4) for r in G16}
    Handle(torch_cuda, fx, rows, masks).round_trip([P], "71 copies")


@pytest.mark.parametrize("knobs", [{"SOLO_ENC_PERSIST": "1"}, {"SOLO_ENC_CHUNK": "0"}, {"SOLO_DEC_SPLIT": "0"}],
                         ids=lambda k: ",".join("%s=%s" % kv for kv in k.items()))
def test_schedule_and_path_variants(torch_cuda, fx, monkeypatch, knobs):
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)                                  # read at the handle's first encode / decode
    for group in ("16k40", "32k40"):
        rows, masks = _rows_x_masks(GROUPS[group])
        Handle(torch_cuda, fx, rows, masks).round_trip([P], "%s %s" % (group, knobs))


def test_per_stream_control_across_the_crossing(torch_cuda, fx):
    """Six streams at row 0's configuration.  0 and 1 are row 0 itself and are never touched; 2, 3, 4 are reset (encoder and decoder) at
    packet 300, at 700 and at both: from there each equals a fresh reference codec, whose VAD counter starts again at 15; 5 goes from
    13600 to 24600 bps at packet 600 and equals a reference encoder whose rate was changed there (tests/ref_ctl_poke.py), its counter
    running on.  The expectations come from the compiled reference (make_long_horizon_golden.py)."""
    import solo_amd
    torch = torch_cuda
    seeds = [int(v) for v in fx["ctl_seeds"]]
    x = np.stack([_input(fx, 0), _input(fx, 0)] + [L.stream_input(np.array((16000, 40, 13600, 0, 0, 0, sd), np.int32), fx["quiet"]) for sd in seeds])
    want_n = np.concatenate([fx["nbytes"][[0, 0]], fx["ctl_nbytes"]])
    want_p = np.concatenate([fx["pcrc"][[0, 0]], fx["ctl_pcrc"]])
    want_d = np.concatenate([fx["dcrc"][0][[0, 0]], fx["ctl_dcrc"]])
    b = solo_amd.SoloBatch(6, rate=13600, encoder=True, decoder=True, slot_bytes=512)
    d_x = _dev(x)
    cuts = [0, 300, L.CTL_RATE_AT, 700, P]
    hb, hn, out = [], [], []
    try:
        for a, e in zip(cuts, cuts[1:]):
            reset = [2 + j for j in range(3) if a in L.CTL_RESETS[j]]
            if reset:
                b.reset_streams(reset, which="both")
            if a == L.CTL_RATE_AT:
                b.update_streams([5], rate=L.CTL_RATE, which="enc")
            bits, nb, st = b.encode(d_x[:, a:e].contiguous())
            y, st2 = b.decode(bits, nb)
            torch.cuda.synchronize()
            assert int(st.abs().max()) == 0 and int(st2.abs().max()) == 0, (a, e)
            hb.append(bits.cpu().numpy()); hn.append(nb.cpu().numpy()); out.append(y.cpu().numpy())
    finally:
        b.close()
    hb, hn, out = np.concatenate(hb, 1), np.concatenate(hn, 1), np.concatenate(out, 1)
    names = ("untouched", "untouched", "reset at 300", "reset at 700", "reset at 300 and 700", "rate change at 600")
    for got, want, what in ((hn, want_n, "lengths"), (_crc_rows(hb, hn[:, :, 0]), want_p, "payload"), (_crc_rows(out), want_d, "PCM")):
        if not np.array_equal(got, want):
            i, p = _first((got != want).reshape(6, P, -1).any(axis=2))
            raise AssertionError("%s: stream %d (%s), packet %d" % (what, i, names[i], p))


@pytest.mark.parametrize("depth", [8, 3])
@pytest.mark.parametrize("group", list(GROUPS))
def test_receiver_ring_over_a_call(torch_cuda, fx, group, depth):
    """A packet's descriptions are sent at tick p and played at tick p + depth - 1.  What mask (b) of the fixture has arrives in time, in
    any order within that window, some of it twice; what it lacks outside the hold arrives after its turn (late), inside the hold
    nothing is sent, an empty DTX packet is never sent.  So the played PCM is the reference decoder's under mask (b), and the per-stream
    counters of solo_recv_track are those of the model (tests/recv_report_model.py) after all 1250 sequence numbers.  Every row of the
    fixture is played, in the handle of its mode."""
    import solo_amd
    torch = torch_cuda
    rows = list(GROUPS[group])
    N, SLOT, BUDGET = len(rows), 256, depth - 1
    enc = Handle(torch, fx, rows, [2] * N)
    try:
        enc.encode([P]).check_encode("ring " + group)
    finally:
        enc.b.close()
    hb, hn, ms = enc.hb, enc.hn, enc.ms
    have = enc.recv()
    rng = np.random.default_rng(100 + depth)
    ticks = [[] for _ in range(P + BUDGET + 4)]
    blobs, off = [], 0
    for i in range(N):
        for p in range(P):
            n0, n1 = int(hn[i, p, 0]), int(hn[i, p, 1])
            if n0 <= 0 or L.HOLD[0] <= p < L.HOLD[1]:
                assert have[i, p] == 0
                continue
            parts = (hb[i, p, :n0 - n1].tobytes(), hb[i, p, n0 - n1:n0].tobytes())
            for d in (0, 1):
                assert 0 < len(parts[d]) <= SLOT
                blobs.append(parts[d])
                if have[i, p] & (1 << d):
                    t = p + int(rng.integers(0, BUDGET + 1))
                    ticks[t].append((i, p, d, off, len(parts[d])))
                    if rng.random() < 0.05:
                        ticks[t + 1].append((i, p, d, off, len(parts[d])))      # once more: a duplicate, or late
                else:
                    ticks[p + BUDGET + 1 + int(rng.integers(0, 3))].append((i, p, d, off, len(parts[d])))
                off += len(parts[d])
    payload = _dev(np.frombuffer(b"".join(blobs), np.uint8).copy())
    cfg = fx["cfg"]
    r0 = cfg[rows[0]]
    b = solo_amd.SoloBatch(N, rate=int(r0[2]), encoder=False, decoder=True, slot_bytes=512, use_md_index=int(r0[3]), joint=int(r0[4]),
                           samplerate=int(r0[0]), framesize_ms=ms)
    try:
        b.reset_streams(list(range(N)), use_md_index=[int(cfg[s][3]) for s in rows], which="dec")
        b.recv_create(depth, SLOT, 0)
        b.recv_track(True)
        m = RingModel(N, depth, SLOT)
        m.track(True)
        got = np.zeros((N, P, b.packet_samples), np.int16)
        for t in range(len(ticks)):
            if ticks[t]:
                arr = [ticks[t][k] for k in rng.permutation(len(ticks[t]))]
                b.recv_insert(torch.tensor(arr, dtype=torch.int32).cuda(), payload)
                m.insert(arr, int(payload.numel()), [0] * N, {})
            if BUDGET <= t < P + BUDGET:
                x, st = b.recv_decode(1)
                torch.cuda.synchronize()
                assert int(st.abs().max()) == 0, t
                got[:, t - BUDGET] = x.cpu().numpy()[:, 0]
                played = m.play_out(range(N), 1)
                for i in range(N):                                    # the model played what mask (b) says had arrived
                    seq, src = played[i][0]
                    assert seq == t - BUDGET and ((1 if src[0] else 0) | (2 if src[1] else 0)) == int(have[i, seq]), (t, i)
        rep = b.recv_report()[0].cpu().numpy()
        want_rep = m.report()[0].astype(np.int32)
        stats = b.recv_stats()
    finally:
        b.close()
    crc, want = _crc_rows(got), fx["dcrc"][2][rows]
    if not np.array_equal(crc, want):
        i, p = _first(crc != want)
        raise AssertionError("ring depth %d: stream %d, arrived %d %s" % (depth, i, int(have[i, p]), L.where(rows[i], p, ms)))
    assert np.array_equal(rep, want_rep), (rep.tolist(), want_rep.tolist())
    assert int(rep[:, 0].min()) == P and stats["late"] > 0 and stats["duplicate"] > 0 and stats["ahead"] == 0 and stats["bad"] == 0, stats
    assert stats["inserted"] == sum(bin(int(v)).count("1") for v in have.ravel())


@pytest.mark.skipif(not R.have_ref("fix"), reason="oracle/_ref not present")
@pytest.mark.parametrize("k", range(len(L.FRESH)))
def test_fresh_seeds_vs_compiled_reference(torch_cuda, k):
    import solo_amd
    torch = torch_cuda
    fs, ms, rate, mdi, joint, dtx = L.FRESH[k]
    seed = 9600 + k
    x = L.stream_input(np.array((fs, ms, rate, mdi, joint, dtx, seed), np.int32), (380, 1150))
    b = solo_amd.SoloBatch(1, rate=rate, encoder=True, decoder=True, slot_bytes=512, use_md_index=mdi, joint=joint, dtx=dtx, samplerate=fs,
                           framesize_ms=ms)
    try:
        bits, nb, st = b.encode(_dev(x[None]))
        torch.cuda.synchronize()
        hb, hn = bits.cpu().numpy()[0], nb.cpu().numpy()[0]
        mask = L.fresh_mask(seed)
        mask[hn[:, 0] <= 0] = 0
        y, st2 = b.decode(bits, nb, _dev(mask[None]))
        torch.cuda.synchronize()
        assert int(st.abs().max()) == 0 and int(st2.abs().max()) == 0
        out = y.cpu().numpy()[0]
    finally:
        b.close()
    kw = dict(samplerate=fs, use_md_index=mdi, joint=joint, framesize_ms=ms)
    er, dr = R.RefEncoder("fix", rate=rate, dtx=dtx, **kw), R.RefDecoder("fix", **kw)
    for p in range(P):
        pl, n0, n1 = er.encode(x[p])
        assert (n0, n1) == (int(hn[p, 0]), int(hn[p, 1])) and hb[p, :n0].tobytes() == pl[:n0], "encoder " + L.where(k, p, ms)
        want, ret = dr.decode(*L.dec_call(pl, n0, n1, int(mask[p])))
        assert ret == 0 and np.array_equal(out[p], want), "decoder, arrived %d %s" % (int(mask[p]), L.where(k, p, ms))

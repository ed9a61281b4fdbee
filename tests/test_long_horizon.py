"""Call-length parity (CPU): the host emulation of the kernel source against tests/golden/long_horizon.npz, the compiled reference's
answers for 1250-packet streams (make_long_horizon_golden.py), packet by packet.

Two things happen only that late.  The VAD noise tracker (solo_enc_front.h, `counter < 1000 ? 32767 / ((counter >> 4) + 1) : 0`) takes
its second arm from SILK frame 985 on (the counter starts at 15; counted from 0: packet 492 of a 40 ms stream, packet 985 of a 20 ms stream).  And the
decoder's concealment / comfort-noise state (lossCnt, hb_lossCnt, randScale_Q14, conc_energy, the CNG smoother, the LCG seeds) is driven
seconds deep only by a call on hold and by minutes on one description: masks (b) and (c) of the fixture.

Every row of the fixture goes through T.EmuEncoder (lengths, payload CRC) and through T.EmuDecoder in both decoder paths (PCM CRC under
the clean decode and the three masks; empty DTX packets are lost packets, as in the reference CLI).  Where oracle/_ref is present two
fresh seeds per mode also run directly against R.RefEncoder / R.RefDecoder.  A failure names (row, packet, VAD frame counter)."""
import os
import zlib

import numpy as np
import pytest

import refcodec as R
import solo_testlib as T

P = 1250
FIXTURE = os.path.join(T.GOLDEN, "long_horizon.npz")
MASK_NAMES = ("clean", "bernoulli30", "hold", "one_description")
VAD_COUNTER_START, VAD_COUNTER_SWITCH = 15, 1000         # solo_enc_state.h, solo_enc_front.h
# the control scenario of tests/test_gpu_long_horizon.py: packets at which control stream j is reset; stream 3 changes its rate instead
CTL_RESETS = ((300,), (700,), (300, 700), ())
CTL_RATE_AT, CTL_RATE = 600, 24600
HOLD = (500, 760)               # mask (b): nothing arrives for 260 packets (10.4 s at 40 ms); elsewhere 2 % of the descriptions are missing


def frames_per_packet(frame_ms):
    return 2 if frame_ms == 40 else 1


def crossing_packet(frame_ms):
    """the first packet (counted from 0) with a frame whose VAD counter has reached 1000: frame f, counted from 0, sees 15 + f"""
    return (VAD_COUNTER_SWITCH - VAD_COUNTER_START) // frames_per_packet(frame_ms)


VOICED_WINDOW, MIN_VOICED = 25, 5    # "voiced packets on both sides of the crossing": at least 5 within 25 packets (1 s / 0.5 s) on either side


def voiced_around_crossing(sigtype, coded, frame_ms):
    """coded packets with a frame the reference called voiced (sigtype 0) in the VOICED_WINDOW packets before the crossing packet and in the
    VOICED_WINDOW from it on; sigtype [P, 2] as the fixture stores it"""
    c = crossing_packet(frame_ms)
    v = (sigtype == 0).any(axis=1) & coded
    return int(v[c - VOICED_WINDOW:c].sum()), int(v[c:c + VOICED_WINDOW].sum())


def packet_samples(fs, frame_ms):
    return 640 * fs // 16000 * frame_ms // 40


def stream_input(row, quiet):
    """int16 [P, samples] of a configuration row (fs, frame_ms, rate, useMDIndex, joint, dtx, seed): the workload generator read at the
    row's packet size (at 32 kHz this is T.synth_stream_32k); DTX rows are near-silent (a few LSBs of noise) over the packets `quiet`"""
    fs, ms, dtx, seed = int(row[0]), int(row[1]), int(row[5]), int(row[6])
    ns = packet_samples(fs, ms)
    x = R.synth_stream(seed, P * ns // 640).reshape(P, ns)
    if dtx:
        x = x.copy()
        a, e = int(quiet[0]), int(quiet[1])
        x[a:e] = (np.random.default_rng(seed).standard_normal((e - a, ns)) * 3).astype(np.int16)
    return np.ascontiguousarray(x)


def dec_call(pl, n0, n1, m):
    """the reference decoder call for one record under the arrival mask m (bit 0: MD1, bit 1: MD2): an empty (DTX) record is a lost
    packet, as in the reference CLI; otherwise the mapping of test/dec_main.c (R.map_loss)"""
    if n0 <= 0:
        return b"", 16, 0, 1
    return R.map_loss(pl[:n0], n0, n1, not (m & 1), not (m & 2))


def load_fixture():
    return np.load(FIXTURE)


def where(row, p, frame_ms):
    return "(row %d, packet %d, VAD frame counter %d)" % (row, p, VAD_COUNTER_START + p * frames_per_packet(frame_ms))


def _flags(row):
    fs, ms, rate, mdi, joint, dtx, seed = (int(v) for v in row)
    return mdi | (joint << 1) | ((1 if ms == 20 else 0) << 3), dtx << 2


_encoded = {}


def emu_encode(row, quiet):
    """the row's 1250 packets from the emulated encoder (kept: the decoder cases of a row start from the same packets)"""
    key = tuple(int(v) for v in row) + tuple(int(v) for v in quiet)
    if key not in _encoded:
        x = stream_input(row, quiet)
        dflags, eflags = _flags(row)
        e = T.EmuEncoder(int(row[2]), dflags | eflags, wb=int(row[0]) == 32000)
        _encoded[key] = [e.encode(x[p]) for p in range(x.shape[0])]
    return _encoded[key]


# The emulation runs one fixture row per mode (16 kHz / 40 ms, 16 kHz / 20 ms, 32 kHz / 40 ms with DTX and useMDIndex, 32 kHz / 20 ms): a row
# costs about 15 s of host time.  SOLO_LONG_HORIZON_ALL=1 runs all ten; tests/test_gpu_long_horizon.py always does.
N_ROWS = 10
ROWS = list(range(N_ROWS)) if os.environ.get("SOLO_LONG_HORIZON_ALL") == "1" else [0, 6, 8, 9]


@pytest.fixture(scope="module")
def fx():
    z = load_fixture()
    assert z["cfg"].shape[0] == N_ROWS and z["nbytes"].shape[1] == P
    return z


def test_crossing_arithmetic():
    assert crossing_packet(40) == 492 and crossing_packet(20) == 985
    for ms in (20, 40):
        c, f = crossing_packet(ms), frames_per_packet(ms)
        assert VAD_COUNTER_START + (c + 1) * f - 1 >= VAD_COUNTER_SWITCH > VAD_COUNTER_START + c * f - 1
        assert c + 250 < P


@pytest.mark.parametrize("s", ROWS)
def test_emulation_encoder_vs_fixture(fx, s):
    row = fx["cfg"][s]
    ms = int(row[1])
    recs = emu_encode(row, fx["quiet"])
    for p, (pl, n0, n1) in enumerate(recs):
        assert (n0, n1) == tuple(int(v) for v in fx["nbytes"][s, p]), "lengths " + where(s, p, ms)
        assert zlib.crc32(pl[:n0]) == int(fx["pcrc"][s, p]), "payload " + where(s, p, ms)


@pytest.mark.parametrize("split", [0, 1], ids=["single", "split"])
@pytest.mark.parametrize("s", ROWS)
def test_emulation_decoder_vs_fixture(fx, s, split):
    """the decoder is fed the emulated encoder's packets where they equal the reference's (checked by CRC), so a decoder failure is the
    decoder's"""
    row = fx["cfg"][s]
    fs, ms = int(row[0]), int(row[1])
    ns = packet_samples(fs, ms)
    recs = emu_encode(row, fx["quiet"])
    ok = all(zlib.crc32(pl[:n0]) == int(fx["pcrc"][s, p]) and n0 == int(fx["nbytes"][s, p, 0]) for p, (pl, n0, n1) in enumerate(recs))
    assert ok, "row %d: the encoder differs (test_emulation_encoder_vs_fixture says where)" % s
    dflags, _ = _flags(row)
    for k, name in enumerate(MASK_NAMES):
        mask = np.full(P, 3, np.uint8) if k == 0 else fx["masks"][k - 1, s]
        d = T.EmuDecoder(dflags, wb=fs == 32000, split=split)
        for p, (pl, n0, n1) in enumerate(recs):
            y, ret = d.decode(*dec_call(pl, n0, n1, int(mask[p])))
            assert ret == 0 and zlib.crc32(y[:ns].tobytes()) == int(fx["dcrc"][k, s, p]), "mask %s (%d) %s" % (name, int(mask[p]), where(s, p, ms))


def test_fixture_covers_what_it_claims(fx):
    cfg, nb, mk = fx["cfg"], fx["nbytes"], fx["masks"]
    modes = {(int(r[0]), int(r[1])) for r in cfg}
    assert modes == {(16000, 40), (16000, 20), (32000, 40), (32000, 20)}
    assert {int(r[0]) for r in cfg if r[5]} == {16000, 32000} and {int(r[3]) for r in cfg} == {0, 1} and any(r[4] for r in cfg)
    for s, r in enumerate(cfg):
        c = crossing_packet(int(r[1]))
        coded = nb[s, :, 0] > 0
        if r[5]:
            assert int((~coded[c:]).sum()) >= 100 and int(coded[c:].sum()) >= 100 and (int(fx["quiet"][1]) - int(fx["quiet"][0])) * int(r[1]) > 30000
        else:
            assert coded.all() and min(voiced_around_crossing(fx["sigtype"][s], coded, int(r[1]))) >= MIN_VOICED
        hold = (mk[1, s] == 0).astype(np.int8)
        runs = np.diff(np.flatnonzero(np.diff(np.concatenate([[0], hold, [0]]))))[::2]
        assert runs.max() >= 250
        assert int((mk[2, s] == 1).sum()) >= 400 and int((mk[2, s] == 2).sum()) >= 400 and mk[2, s, -1] == 3
        assert {int(v) for v in mk[0, s]} == {0, 1, 2, 3}
    assert os.path.getsize(FIXTURE) <= os.path.getsize(os.path.join(T.GOLDEN, "synth8x25.npz"))


FRESH = [(16000, 40, 13600, 1, 0, 0), (16000, 40, 20000, 0, 1, 1), (16000, 20, 13600, 1, 0, 0), (16000, 20, 24000, 0, 0, 1),
         (32000, 40, 24000, 1, 0, 0), (32000, 40, 30000, 0, 0, 1), (32000, 20, 24000, 1, 0, 0), (32000, 20, 15600, 0, 0, 0)]


def fresh_mask(seed):
    """30 % loss per description, a hold of 300 packets and 420 packets on either description alone, in one mask"""
    m = T.bernoulli_recv(1, P, 0.3, seed)[0]
    m[150:450] = 0
    m[520:940] &= 1
    m[600:700] = 1
    m[940:1240] &= 2
    m[1000:1100] = 2
    return m


@pytest.mark.skipif(not R.have_ref("fix"), reason="oracle/_ref not built")
@pytest.mark.parametrize("k", range(len(FRESH)))
def test_emulation_vs_compiled_reference_fresh_seeds(k):
    fs, ms, rate, mdi, joint, dtx = FRESH[k]
    seed = 9500 + k
    row = np.array((fs, ms, rate, mdi, joint, dtx, seed), np.int32)
    ns = packet_samples(fs, ms)
    x = stream_input(row, (380, 1150))
    kw = dict(samplerate=fs, use_md_index=mdi, joint=joint, framesize_ms=ms)
    er = R.RefEncoder("fix", rate=rate, dtx=dtx, **kw)
    dflags, eflags = _flags(row)
    ee = T.EmuEncoder(rate, dflags | eflags, wb=fs == 32000)
    recs = []
    for p in range(P):
        want, got = er.encode(x[p]), ee.encode(x[p])
        assert got[1:] == want[1:] and got[0][:want[1]] == want[0][:want[1]], "encoder " + where(k, p, ms)
        recs.append(want)
    mask = fresh_mask(seed)
    dr = R.RefDecoder("fix", **kw)
    de = [T.EmuDecoder(dflags, wb=fs == 32000, split=sp) for sp in (0, 1)]
    for p, (pl, n0, n1) in enumerate(recs):
        a = dec_call(pl, n0, n1, int(mask[p]))
        want, rw = dr.decode(*a)
        assert rw == 0
        for sp in (0, 1):
            got, rg = de[sp].decode(*a)
            assert rg == 0 and np.array_equal(got[:ns], want), "decoder path %d, lostflag %d %s" % (sp, a[3], where(k, p, ms))

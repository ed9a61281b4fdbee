"""The all-pass chains at the front of the analysis kernel (solo_enc_front.h: sx_allpass2_spread / sx_allpass2_chain and their finish passes --
the VAD's three filter banks and the pitch analysis decimators) on inputs chosen to break exactly them, at 16 kHz and 32 kHz, 8 streams x 4 packets:

 * full-scale squares of +-32767 with periods of 2, 4 and 8 samples: the first is all high band (the chains see the QMF's transients and then
   zeros), the other two put full-scale tones at the top of the QMF's low band and at the first filter bank's crossover, which drives the band
   sums of the finish passes -- also of the low band a finish pass hands on to the next bank's chains -- to the 16-bit limit that sat16 guards;
 * all zeros;
 * DC steps (0 -> 30000 in mid-packet; -32768 -> 32767 at an odd sample: both band sums at the limit before the step, overshoot after it);
 * synthetic speech (solo_amd.synth).

Every input runs two ways -- one call of 4 packets, four calls of 1 packet -- through the solo_debug_analysis probe (launches of 4 and of 1 packets)
and through SoloBatch.encode: the chain states cross frame, packet, launch and call boundaries.  The two ways must agree byte for byte, whatever
else is present; where oracle/_ref holds the compiled reference (its tap build, loaded through oracle/refcodec.py), every hand-over field and
every payload byte must equal the reference's as well (masks and record layouts: tests/test_enc_stages.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

import refcodec as R
import solo_testlib as T  # noqa: F401  (puts the repository on sys.path)
import test_enc_stages as ES
from solo_amd.synth import synth_stream

N, P = 8, 4
RATES = {"nb": (16000, 13600), "wb": (32000, 24000)}          # API sample rate, targetRate_bps
SLOT = 1024
NEED_REF = pytest.mark.skipif(not R.have_ref("fix_taps"), reason="no compiled reference (oracle/_ref/libsolo_ref_fix_taps.so) on this machine")


@functools.lru_cache(None)
def _pcm(rate):
    """int16 [N][P][packet samples]"""
    L = 640 * RATES[rate][0] // 16000
    t = np.arange(P * L)
    x = np.zeros((N, P * L), np.int16)
    for i, period in enumerate((2, 4, 8)):
        x[i] = np.where((t // (period // 2)) % 2 == 0, 32767, -32767)
    # x[3]: zeros
    x[4, P * L * 3 // 8:] = 30000
    x[5] = np.where(t < 2 * L + 77, -32768, 32767)
    for i in (6, 7):
        x[i] = synth_stream(4730 + i, P * L // 640).reshape(-1)
    x = np.ascontiguousarray(x.reshape(N, P, L))
    x.setflags(write=False)
    return x


def _init(rate):
    sr, total = RATES[rate]
    return (sr, total - 1600, 0, 0, 0, 2)                      # (as tests/test_enc_stages.py: AGR_BWE_SDK_API.c:119)


@functools.lru_cache(None)
def _reference(rate):
    """per stream: the reference's SxNsqIn [P][2], SxCodeIn [P], the comparison masks, payloads and byte counts (tests/golden/make_enc_stages.py)"""
    sr, total = RATES[rate]
    wb = rate == "wb"
    nsq_in_dt, idx_dt, code_dt = ES._dtypes(wb)[:3]
    lib = C.CDLL(R.ref_lib_path("fix_taps"))
    lib.AGR_Sate_Encoder_Init.restype = C.c_void_p
    lib.AGR_Sate_Encoder_Init.argtypes = [C.c_void_p]
    lib.AGR_Sate_Encoder_Encode.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    lib.AGR_Sate_Encoder_Uninit.argtypes = [C.c_void_p]
    counts = [C.c_int.in_dll(lib, n) for n in ("solo_nsq_tap_n", "solo_idx_tap_n", "solo_hi_tap_n")]
    tap_in = (C.c_ubyte * (512 * 980)).in_dll(lib, "solo_nsq_tap_in")
    tap_idx = (C.c_int32 * (512 * 32)).in_dll(lib, "solo_idx_tap")
    tap_hi = (C.c_int16 * (64 * 640)).in_dll(lib, "solo_hi_tap")
    idx_ints = C.c_int.in_dll(lib, "solo_idx_tap_ints")
    pcm = _pcm(rate)
    band = pcm.shape[2] // 2
    out = []
    for i in range(N):
        for c in counts:
            c.value = 0
        ctrl = R.default_enc_ctrl(total, samplerate=sr)
        h = lib.AGR_Sate_Encoder_Init(C.byref(ctrl))
        assert h
        buf, nb = np.zeros(2048, np.uint8), np.zeros(6, np.int16)
        pay, nbytes = [], np.zeros((P, 2), np.int16)
        for p in range(P):
            x = np.ascontiguousarray(pcm[i, p])
            nb[:] = 0
            n = lib.AGR_Sate_Encoder_Encode(h, x.ctypes.data, buf.ctypes.data, 2048, nb.ctypes.data)
            nbytes[p] = nb[:2]
            pay.append(buf[:n].copy())
        lib.AGR_Sate_Encoder_Uninit(h)
        si, ni = lib.solo_nsq_tap_sizeof_in(), idx_ints.value                      # (both set while the reference runs)
        assert [c.value for c in counts] == [2 * P, 2 * P, P * band] and si == nsq_in_dt.itemsize and 4 * ni == idx_dt.itemsize
        raw_in = np.frombuffer(tap_in, np.uint8, 2 * P * si).reshape(P, 2, si).copy()
        raw_in[..., 20:24][raw_in[..., 0:4].view("<i4")[..., 0] != 0] = 0          # LTP_scale_Q14 of unvoiced frames: undefined in the reference, zero here
        cin = np.zeros(P, code_dt)
        cin["idx"] = np.frombuffer(tap_idx, np.int32, 2 * P * 32).reshape(P, 2, 32)[:, :, :ni].copy().view(idx_dt).reshape(P, 2)
        cin["hi"][:, :band] = np.frombuffer(tap_hi, np.int16, P * band).reshape(P, band)
        m_in, m_cin = ES._masks(wb, 2, cin)
        out.append(dict(k=i, nsq_in=raw_in.view(nsq_in_dt).reshape(P, 2), cin=cin, mask_in=m_in, mask_cin=m_cin, pay=pay, nbytes=nbytes))
    return out


@functools.lru_cache(None)
def _probe(rate, chunk):
    """solo_debug_analysis in launches of `chunk` packets (0: all of them) -> SxNsqIn [N][P][2], SxCodeIn [N][P]"""
    import solo_amd
    lib = solo_amd.load_library()
    nsq_in_dt, _, code_dt = ES._dtypes(rate == "wb")[:3]
    pcm = _pcm(rate)
    got_in, got_cin = np.zeros((N, P, 2), nsq_in_dt), np.zeros((N, P), code_dt)
    assert lib.solo_debug_analysis(*_init(rate), N, P, chunk, pcm.ctypes.data, got_in.ctypes.data, got_cin.ctypes.data, None) == nsq_in_dt.itemsize
    return got_in, got_cin


@functools.lru_cache(None)
def _encode(rate, per_call):
    """SoloBatch.encode in calls of `per_call` packets -> bits uint8 [N][P][SLOT], nbytes int16 [N][P][2]"""
    import torch
    import solo_amd
    sr, total = RATES[rate]
    b = solo_amd.SoloBatch(N, rate=total, encoder=True, decoder=False, slot_bytes=SLOT, samplerate=sr)
    pcm = torch.from_numpy(np.array(_pcm(rate))).cuda()
    bits, nbytes = [], []
    for p in range(0, P, per_call):
        bi, nb, st = b.encode(pcm[:, p:p + per_call].contiguous())
        torch.cuda.synchronize()
        assert int(st.abs().max()) == 0
        bits.append(bi.cpu().numpy().copy())
        nbytes.append(nb.cpu().numpy().copy())
    return np.concatenate(bits, axis=1), np.concatenate(nbytes, axis=1)


@pytest.mark.gpu
@pytest.mark.parametrize("rate", list(RATES))
def test_probe_launches_of_one_packet_equal_one_launch_of_four(rate):
    for a, b, nm in zip(_probe(rate, 0), _probe(rate, 1), ("SxNsqIn", "SxCodeIn")):
        d = np.nonzero(a.view(np.uint8).reshape(N, P, -1) != b.view(np.uint8).reshape(N, P, -1))
        assert d[0].size == 0, (rate, nm, "stream %d packet %d byte %d" % (d[0][0], d[1][0], d[2][0]))


@pytest.mark.gpu
@pytest.mark.parametrize("rate", list(RATES))
def test_encode_calls_of_one_packet_equal_one_call_of_four(rate):
    (bits4, nb4), (bits1, nb1) = _encode(rate, P), _encode(rate, 1)
    assert np.array_equal(nb4, nb1), (rate, "byte counts", np.argwhere(nb4 != nb1)[0])
    assert nb4[..., 0].min() > 0
    for i in range(N):
        for p in range(P):
            n = int(nb4[i, p, 0])
            assert np.array_equal(bits4[i, p, :n], bits1[i, p, :n]), (rate, "payload of stream %d packet %d" % (i, p))


@pytest.mark.gpu
@NEED_REF
@pytest.mark.parametrize("rate", list(RATES))
def test_probe_equals_the_reference_field_by_field(rate):
    got_in, got_cin = _probe(rate, 0)
    for s in _reference(rate):
        ES._check_a(s, rate, got_in[s["k"]], got_cin[s["k"]], "%s stream %d" % (rate, s["k"]))


@pytest.mark.gpu
@NEED_REF
@pytest.mark.parametrize("rate", list(RATES))
def test_encode_equals_the_reference_payloads(rate):
    bits, nb = _encode(rate, P)
    for s in _reference(rate):
        i = s["k"]
        assert np.array_equal(nb[i], s["nbytes"]), (rate, "byte counts of stream %d" % i, nb[i].tolist(), s["nbytes"].tolist())
        for p in range(P):
            n = int(s["nbytes"][p, 0])
            assert n > 0 and bits[i, p, :n].tobytes() == s["pay"][p][:n].tobytes(), (rate, "payload of stream %d packet %d" % (i, p))

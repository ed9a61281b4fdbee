#!/usr/bin/env python3
"""Makes tests/golden/enc_stages.npz (16 kHz API rate) and tests/golden/enc_stages_wb.npz (32 kHz): what the compiled reference hands from
stage to stage of its encoder, packet by packet, for streams chosen because each reaches a path whose result only SOME consumer reads
(STREAMS / STREAMS_WB below).  Per stream `k` (keys "sKK_*"): the input PCM, the arguments of every SKP_Silk_NSQ_del_dec call in the layout of
SxNsqIn (`nsq_in`), the coded indices of every frame in the field order of SxFrameIdx (`idx`), the high band the QMF analysis hands to the
high-band encoder (`hi`), the quantiser's outputs (`nsq_out`: {int32 Seed; int8 q[2][L]; int32 r[L]}), and the payload: `bits`, `nbytes`
(what AGR_Sate_Encoder_Encode writes to nBytesOut[0..1]) and `nret` (what it returns: the bytes it wrote, which is the high band's alone
for a packet dropped by DTX).  `params` rows: (samplerate, targetRate_bps, useMDIndex, joint, dtx, framesize_ms, packets).

Needs oracle/_ref/libsolo_ref_fix_taps.so (`make -C oracle taps`: the unmodified reference linked with oracle/ref_taps.c through
-Wl,--wrap), i.e. runs only where the reference sources are; the files it writes are data and travel.  tests/test_enc_stages.py runs the
analysis stage and the coding stage ALONE on these records and compares."""
import ctypes as C
import os
import sys
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), ROOT]
import refcodec as R
import solo_testlib as T
from solo_amd.synth import edge_stream

lib = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libsolo_ref_fix_taps.so"))
lib.AGR_Sate_Encoder_Init.restype = C.c_void_p
lib.AGR_Sate_Encoder_Init.argtypes = [C.c_void_p]
lib.AGR_Sate_Encoder_Encode.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
lib.AGR_Sate_Encoder_Uninit.argtypes = [C.c_void_p]
nsq_n = C.c_int.in_dll(lib, "solo_nsq_tap_n")
idx_n = C.c_int.in_dll(lib, "solo_idx_tap_n")
idx_ints = C.c_int.in_dll(lib, "solo_idx_tap_ints")
hi_n = C.c_int.in_dll(lib, "solo_hi_tap_n")
tap_in = (C.c_ubyte * (512 * 980)).in_dll(lib, "solo_nsq_tap_in")
tap_out = (C.c_ubyte * (512 * 1924)).in_dll(lib, "solo_nsq_tap_out")
tap_idx = (C.c_int32 * (512 * 32)).in_dll(lib, "solo_idx_tap")
tap_hi = (C.c_int16 * (64 * 640)).in_dll(lib, "solo_hi_tap")


def run(pcm, rate=13600, md=0, joint=0, dtx=0, samplerate=16000, ms=40):
    """pcm [P, packet samples] -> the records of one freshly initialised reference encoder"""
    P, L = pcm.shape
    fpp, band = ms // 20, L // 2
    assert L == samplerate // 1000 * ms and P <= 64
    nsq_n.value = idx_n.value = hi_n.value = 0
    ctrl = R.default_enc_ctrl(rate, use_md_index=md, joint=joint, dtx=dtx, samplerate=samplerate, framesize_ms=ms)
    h = lib.AGR_Sate_Encoder_Init(C.byref(ctrl))
    buf, nb = np.zeros(2048, np.uint8), np.zeros(6, np.int16)
    pay, nbytes, nret = [], np.zeros((P, 2), np.int16), np.zeros(P, np.int16)
    for p in range(P):
        x = np.ascontiguousarray(pcm[p])
        nb[:] = 0
        nret[p] = lib.AGR_Sate_Encoder_Encode(h, x.ctypes.data, buf.ctypes.data, 2048, nb.ctypes.data)
        nbytes[p] = nb[:2]
        pay.append(buf[:nret[p]].copy())
    lib.AGR_Sate_Encoder_Uninit(h)
    n = P * fpp
    assert nsq_n.value == n and idx_n.value == n and hi_n.value == P * band, (nsq_n.value, idx_n.value, hi_n.value)
    si, so, ni = lib.solo_nsq_tap_sizeof_in(), lib.solo_nsq_tap_sizeof_out(), idx_ints.value
    assert si == 340 + band // fpp * 2 and ni == (26 if samplerate == 16000 else 30), (si, ni)

    def rows(buf_, dt, width, stride=None):  # [P, 2, width]: the second record of a one-frame packet stays zero
        a = np.zeros((P, 2, width), dt)
        a[:, :fpp] = np.frombuffer(buf_, dt, n * (stride or width)).reshape(P, fpp, stride or width)[:, :, :width]
        return a
    nsq_in = rows(tap_in, np.uint8, si)
    # LTP_scale_Q14 (bytes 20..23 of SxNsqIn) of an UNVOICED frame (sigtype, bytes 0..3, != 0): assigned in the voiced branch alone
    # (SKP_Silk_LTP_scale_ctrl_FIX.c:80, called from SKP_Silk_find_pred_coefs_FIX.c:87), so the quantiser is handed whatever the stack held:
    # zeroed, like the prediction coefficients beyond the LPC order, so that the file is a function of the input alone
    nsq_in[..., 20:24][nsq_in[..., 0:4].view("<i4")[..., 0] != 0] = 0
    bits = np.zeros((P, max(int(nret.max()), 1)), np.uint8)
    for p in range(P):
        bits[p, :nret[p]] = pay[p]
    return dict(pcm=pcm.copy(), nsq_in=nsq_in, nsq_out=rows(tap_out, np.uint8, so), idx=rows(tap_idx, np.int32, ni, 32),
                hi=np.frombuffer(tap_hi, np.int16, P * band).reshape(P, band).copy(), bits=bits, nbytes=nbytes, nret=nret,
                params=np.array([samplerate, rate, md, joint, dtx, ms, P], np.int32))


def dtx_pcm():      # speech, 24 packets of near-silence, speech (tests/test_gpu_encoder.py: test_dtx_round_trip_vs_compiled_reference, stream 0)
    x = R.synth_stream(800, 40)
    x[3:27] = (np.random.default_rng(9).standard_normal((24, 640)) * 3).astype(np.int16)
    return x


P = 20                              # (24 packets per stream put the file above the largest committed fixture)
# (name, PCM, arguments of run): what each stream is in the file for
STREAMS = [
    ("ch_f1: Ch_f1_raw.pcm packets 0..39, voiced / unvoiced transitions of real speech", T.load_ch_f1()[:40 * 640].reshape(40, 640), {}),
    ("synth: synth_stream(4711)", R.synth_stream(4711, P), {}),
    ("silence: edge_stream(0), zero energy with stray LSBs", edge_stream(0, P), {}),
    ("square: edge_stream(2), full scale", edge_stream(2, P), {}),
    ("sweep: edge_stream(9)", edge_stream(9, P), {}),
    ("hb_tone: edge_stream(10), everything in the high band", edge_stream(10, P), {}),
    ("impulses: edge_stream(4)", edge_stream(4, P), {}),
    ("sweep_hi: edge_stream(9) at 101600 bps, the upper rate clamp", edge_stream(9, P), dict(rate=101600)),
    ("sweep_lo: edge_stream(9) at 6600 bps, the lower rate clamp", edge_stream(9, P), dict(rate=6600)),
    ("dtx: synth_stream(800) with packets 3..26 replaced by noise of sigma 3 (default_rng(9)), dtx=1", dtx_pcm(), dict(dtx=1)),
    ("joint: synth_stream(4712), joint=1", R.synth_stream(4712, P), dict(joint=1)),
    ("fs20: synth_stream(4713) in packets of 20 ms, framesize_ms=20", R.synth_stream(4713, P // 2).reshape(P, 320), dict(ms=20)),
    ("mdindex: synth_stream(4714), useMDIndex=1", R.synth_stream(4714, P), dict(md=1)),
]
PW = 16
WB = dict(samplerate=32000, rate=24000)
STREAMS_WB = [
    ("synth: synth_stream(4721) read at 32 kHz", R.synth_stream(4721, 2 * PW).reshape(PW, 1280), WB),
    ("sweep: edge_stream(9) read at 32 kHz", edge_stream(9, 2 * PW).reshape(PW, 1280), WB),
    ("square_hi: edge_stream(30) read at 32 kHz, 101600 bps, the upper rate clamp (edge_stream(2) stays at |q| 16; edge_stream(16) overflows the reference's stack)", edge_stream(30, 2 * PW).reshape(PW, 1280), dict(samplerate=32000, rate=101600)),
    ("silence: edge_stream(0) read at 32 kHz", edge_stream(0, 2 * PW).reshape(PW, 1280), WB),
]


def facts(recs):
    """what the fixture is for, counted from its records (tests/test_enc_stages.py counts again from the file)"""
    both = trans_vu = trans_uv = dropped = 0
    interp = set()
    for r in recs:
        fpp = int(r["params"][5]) // 20
        sig = r["idx"][:, :fpp, 0]
        both += int((sig == 0).any() and (sig == 1).any())
        if fpp == 2:
            trans_vu += int(((sig[:, 0] == 0) & (sig[:, 1] == 1)).sum())
            trans_uv += int(((sig[:, 0] == 1) & (sig[:, 1] == 0)).sum())
        if r["params"][4]:
            dropped += int((r["nbytes"][:, 0] == 0).sum())
        ni = r["idx"].shape[2]
        interp |= set(int(v) for v in r["idx"][:, :fpp, ni - 13].reshape(-1))
    return both, trans_vu, trans_uv, dropped, interp


def qmax(r):
    L = (r["nsq_out"].shape[2] - 4) // 6
    return int(np.abs(r["nsq_out"][:, :int(r["params"][5]) // 20, 4:4 + 2 * L].view(np.int8).astype(np.int32)).max())


def write(name, streams, wb):
    recs = [run(x, **kw) for _, x, kw in streams]
    both, tvu, tuv, dropped, interp = facts(recs)
    clamps = [qmax(r) for (n, _, _), r in zip(streams, recs) if "clamp" in n]
    print(name, "both signal types in %d streams, transitions inside a packet v->u %d u->v %d, dropped %d, interpolation factors %s, clamp |q| %s"
          % (both, tvu, tuv, dropped, sorted(interp), clamps))
    if not wb:
        assert both >= 4 and tvu >= 1 and tuv >= 1 and dropped >= 8 and 4 in interp and min(interp) < 4
    assert min(clamps) >= 20, clamps
    out = {}
    for k, r in enumerate(recs):
        for f, v in r.items():
            out["s%02d_%s" % (k, f)] = v
    note = ("streams: " + "; ".join("s%02d = %s" % (k, n) for k, (n, _, _) in enumerate(streams)) + ".  Per stream: pcm [P][packet samples], "
            "nsq_in [P][2] rows = struct SxNsqIn, idx [P][2] rows = struct SxFrameIdx (Seed: the one the quantiser was called with), hi [P][band], "
            "nsq_out [P][2] rows = {int32 Seed; int8 q[2][L]; int32 r[L]} of the reference, bits / nbytes / nret of AGR_Sate_Encoder_Encode, "
            "params = (samplerate, targetRate_bps, useMDIndex, joint, dtx, framesize_ms, P).  largest |q| of the clamp streams %d" % max(clamps))
    np.savez_compressed(os.path.join(HERE, name), n_streams=np.int32(len(recs)), note=np.array(note), **out)
    print("wrote", name, os.path.getsize(os.path.join(HERE, name)), "bytes")


if __name__ == "__main__":
    write("enc_stages.npz", STREAMS, False)
    write("enc_stages_wb.npz", STREAMS_WB, True)

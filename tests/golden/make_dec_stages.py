#!/usr/bin/env python3
"""Makes tests/golden/dec_stages.npz (16 kHz API rate) and tests/golden/dec_stages_wb.npz (32 kHz): what the compiled reference DECODER holds
at every stage boundary, packet by packet, for streams and receive masks chosen because each reaches a path that shapes PCM only much later, if
at all (STREAMS / STREAMS_WB below).  Per stream `k` (keys "sKK_*"):
  params   (samplerate, targetRate_bps, useMDIndex, joint, dtx, framesize_ms, packets, corrupted packet or -1, its reason or 0)
  bits / nbytes / recv   what solo_batch_decode is handed: the reference encoder's payloads (one of them corrupted, see below), its byte counts,
           the receive mask (bit 0: description 1 arrived, bit 1: description 2)
  pcm / ret   AGR_Sate_Decoder_Decode's output and return code for every packet, called as the batched API maps the record (dec_stages_lib.map_record)
  ext      [P][2] expected SxExtracted records (solo_amd/csrc/solo_dec.h), packed from the taps of oracle/ref_taps_dec.c: symbols, pulses, control
           blocks, gain indices of the two SKP_Silk_decode_parameters calls per description, the prediction coefficients and the high band's side
           information for the slot that carries them; zero where the reference has no value
  meta     [P] (lostflag, moreInternalDecoderFrames before the call, state recorded (the decoder left its initial 24 kHz), parameter calls tapped,
           every tapped frame read to its end, first_frame_after_reset before the packet's first frame)
  state    [P] SxDecState after the call, from the reference's decoder, PLC, CNG and high-band state (zero while `state recorded` is 0)

Corrupted descriptions: searched with the mutations of tools/debug/fuzz_decoder_gen.py (random bytes, a burst, a bit flip inside one description
of packet 3 of a clean stream), through the host emulation's extraction step (emu_dec_extract), until for every reason a record is unusable --
coder error, fs_bad, narrow, ambiguous, and two usable records whose frames announce another number of frames than the ordinary packet
(structure) -- one input is found that the reference decodes without crashing (tried in a child process); at most TRIALS mutations per rate.
The seed and the number of trials each reason took are printed and kept in the file's `note`, and so is every reason that was NOT found: no
input built to fit stands in for it.

Self-checks (asserted here, counted again from the files by tests/test_dec_stages.py): every lostflag 1..4 occurs, a burst of >= 6 lost packets,
leading loss, >= 6 packets of lostflag 2 only and of lostflag 3 only, CNG active in some packet, both signal types, NLSF interpolation on and
off, every clean received description of a two-frame stream usable by the rule of sx_extracted_usable, every reason found present.

Needs oracle/_ref/libsolo_ref_fix_taps.so (`make -C oracle taps`) and the host emulation; runs only where the reference sources are.  The files
hold data only and are reproduced byte for byte."""
import ctypes as C
import os
import sys
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), ROOT]
import refcodec as R
import solo_testlib as T
import dec_stages_lib as L
from solo_amd.synth import edge_stream

TRIALS = 50000
SEED = 20261
lib = R.load_ref("fix_taps")
g = lambda n, t: t.in_dll(lib, n)
tap_rec = (C.c_int32 * (160 * L.DREC_INTS)).in_dll(lib, "solo_dec_tap_rec")
tap_state = (C.c_int32 * (40 * 4096)).in_dll(lib, "solo_dec_tap_state")
tap_hb = (C.c_int32 * (80 * 20)).in_dll(lib, "solo_dec_tap_hb")


def encode(pcm, rate=13600, md=0, joint=0, dtx=0, samplerate=16000, ms=40):
    e = R.RefEncoder("fix", rate=rate, joint=joint, dtx=dtx, samplerate=samplerate, use_md_index=md, framesize_ms=ms)
    recs = [e.encode(x) for x in pcm]
    e.close()
    return recs


def hb_bytes(joint, ms):
    return 4 if (joint or ms == 20) else 8


def decode(recs, recv, md=0, joint=0, samplerate=16000, ms=40, wide=False, **_):
    """the reference decoder, one packet per tap run -> pcm, ret, ext, meta, state of every packet"""
    wb = samplerate == 32000
    dt = L.dtypes(wb)
    fs, F, lpc = (16, 320, 16) if wb else (8, 160, 10)
    fpp, hbb = ms // 20, hb_bytes(joint, ms)
    d = R.RefDecoder("fix_taps", joint=joint, samplerate=samplerate, use_md_index=md, framesize_ms=ms)
    P = len(recs)
    pcm, ret = np.zeros((P, d.packet_samples), np.int16), np.zeros(P, np.int32)
    ext, meta, state = np.zeros((P, 2), dt["ext"]), np.zeros((P, 6), np.int32), np.zeros(P, dt["state"])
    more = 0
    for p, (pl, n0, n1) in enumerate(recs):
        off, a0, a1, lostflag = L.map_record(n0, n1, int(recv[p]), hbb)
        lib.solo_dec_tap_reset(fs)
        pcm[p], ret[p] = d.decode(pl[off:off + a0] if lostflag != 1 else b"", a0, a1, lostflag)
        n = g("solo_dec_tap_n", C.c_int).value
        assert g("solo_dec_tap_state_n", C.c_int).value == 1 and n <= 8
        r = np.frombuffer(tap_rec, np.int32, n * L.DREC_INTS).reshape(n, L.DREC_INTS)
        hb = np.frombuffer(tap_hb, np.int32, 40).reshape(2, 20)
        s = np.frombuffer(tap_state, np.int32, g("solo_dec_tap_state_ints", C.c_int).value)
        assert s[0] == ret[p]
        meta[p] = (lostflag, more, s[1], n, int(n > 0 and r[:, 4].all()), int(r[0, 3]) if n else 0)
        if s[1]:
            state[p], used = L.unflatten(s[2:], dt["state"], skip=("last_error", "dbg"))
            assert used == s.size - 2, (used, s.size)
            more = int(state[p]["moreInternalDecoderFrames"])
        ndesc = 2 if lostflag == 4 else (1 if lostflag >= 2 else 0)
        # an ordinary two-frame packet: the calls come as (frame 0, description 0), [(0, 1)], (1, 0), [(1, 1)]
        if (fpp == 2 and ndesc and meta[p, 1] == 0 and n == 2 * ndesc and r[:, 4].all() and ret[p] == 0
                and (not wide or [tuple(v) for v in r[:, :2]] == [(f, k) for f in range(2) for k in range(ndesc)])):
            assert [tuple(v) for v in r[:, :2]] == [(f, k) for f in range(2) for k in range(ndesc)]
            for k in range(ndesc):
                e = ext[p, k]
                if wide and max(np.abs(r[f * ndesc + k][L.DREC_PULSES:L.DREC_PULSES + F]).max() for f in range(2)) > 127:
                    e["pad_"][0] = L.NARROW     # (make_dec_constructed.py: SxExtracted::pulses cannot hold them -- no record of this description)
                    continue
                for f in range(2):
                    q = r[f * ndesc + k]
                    e["y"][f] = L.unflatten(q[L.DREC_SYMS:], dt["syms"])[0]
                    assert np.abs(q[L.DREC_PULSES:L.DREC_PULSES + F]).max() <= 127
                    e["pulses"][f] = q[L.DREC_PULSES:L.DREC_PULSES + F]
                    e["ctl"][f] = L.unflatten(q[L.DREC_CTL:], dt["ctl"])[0]
                    e["lastGain"][f] = q[L.DREC_CTL + 37]
                if k == ndesc - 1:          # the slot the decoder takes its coefficients (and the high band) from
                    e["have_A"] = 1
                    for f in range(2):
                        q = r[f * ndesc + k]
                        e["A_final"][f] = q[L.DREC_A + 1:L.DREC_A + 17]
                    q = r[ndesc + k]
                    if q[L.DREC_A] == 2:    # frame 1 interpolated between the packet's two vectors
                        e["A_interp1"] = q[L.DREC_A + 17:L.DREC_A + 33]
                    if lostflag != 2:
                        e["have_hb"] = 1
                        for f in range(1 if hbb == 4 else 2):
                            e["hb_lsp"][f], e["hb_lpc"][f], e["hb_gain"][f] = hb[f, :8], hb[f, 8:16], hb[f, 16:20]
                e["usable"] = 1
        elif fpp == 1 and ndesc and n >= ndesc and r[:ndesc, 4].all():
            for k in range(ndesc):          # a 20 ms packet: its one frame (decoded twice; the first time counts)
                ext[p, k]["y"][0] = L.unflatten(r[k][L.DREC_SYMS:], dt["syms"])[0]
                ext[p, k]["pulses"][0] = r[k][L.DREC_PULSES:L.DREC_PULSES + F]
    d.close()
    return pcm, ret, ext, meta, state


def masks(P, kind, seed):
    """receive masks [P] (bit 0: description 1 arrived, bit 1: description 2)"""
    m = np.full(P, 3, np.uint8)
    rng = np.random.default_rng(seed)
    if kind == "mix":                           # every lostflag, singly and in pairs
        m[:] = rng.choice([3, 3, 1, 2, 0], P)
        m[0] = 3
        m[2:6] = (1, 2, 0, 3)
    elif kind == "burst":                       # seven packets lost in a row: PLC attenuation, CNG
        m[4:11] = 0
    elif kind == "lead":                        # nothing before packet 2, then a mix
        m[:] = rng.choice([3, 1, 2, 0], P)
        m[:2] = 0
        m[2] = 3
    elif kind == "md1":                         # minutes on description 1 in miniature
        m[3:11] = 1
    elif kind == "md2":
        m[3:11] = 2
    elif kind == "lead1":                       # the first packet that arrives carries one description
        m[0] = 0
        m[1] = 2
        m[5] = 1
    return m


P = 16
SP = lambda seed, n=P: R.synth_stream(seed, n)
# (name, PCM, encoder / decoder arguments, mask kind)
STREAMS = [
    ("ch_f1: Ch_f1_raw.pcm packets 20..35, mix of all lostflags", T.load_ch_f1()[20 * 640:36 * 640].reshape(16, 640), {}, "mix"),
    ("synth_burst: synth_stream(5101), seven packets lost in a row", SP(5101), {}, "burst"),
    ("synth_lead: synth_stream(5102), leading loss", SP(5102), {}, "lead"),
    ("hi_md1: synth_stream(5103) at 101600 bps (upper clamp), eight packets of description 1 only", SP(5103), dict(rate=101600), "md1"),
    ("lo_md2: synth_stream(5104) at 6600 bps (lower clamp), eight packets of description 2 only", SP(5104), dict(rate=6600), "md2"),
    ("silence_burst: edge_stream(0), burst", edge_stream(0, P), {}, "burst"),
    ("square_mix: edge_stream(2), full scale", edge_stream(2, P), {}, "mix"),
    ("sweep_lead1: edge_stream(9), first arrival is a lone description 2", edge_stream(9, P), {}, "lead1"),
    ("mdindex_mix: synth_stream(5105), useMDIndex=1", SP(5105), dict(md=1), "mix"),
    ("joint_mix: synth_stream(5106), joint=1", SP(5106), dict(joint=1), "mix"),
    ("fs20_mix: synth_stream(5107) in packets of 20 ms", SP(5107, P // 2).reshape(P, 320), dict(ms=20), "mix"),
    ("dtx_burst: synth_stream(800) with packets 3..12 replaced by noise of sigma 3 (default_rng(9)), dtx=1: empty records", None, dict(dtx=1), "lead1"),
]
PW = 12
WB = dict(samplerate=32000, rate=24000)
STREAMS_WB = [
    ("synth_mix: synth_stream(5121) read at 32 kHz", SP(5121, 2 * PW).reshape(PW, 1280), WB, "mix"),
    ("synth_burst: synth_stream(5122) read at 32 kHz", SP(5122, 2 * PW).reshape(PW, 1280), WB, "burst"),
    ("sweep_md1: edge_stream(9) read at 32 kHz, 101600 bps", edge_stream(9, 2 * PW).reshape(PW, 1280), dict(samplerate=32000, rate=101600), "md1"),
    ("mdindex_md2: synth_stream(5123) read at 32 kHz, useMDIndex=1", SP(5123, 2 * PW).reshape(PW, 1280), dict(samplerate=32000, rate=24000, md=1), "md2"),
]


def dtx_pcm():
    x = R.synth_stream(800, P)
    x[3:13] = (np.random.default_rng(9).standard_normal((10, 640)) * 3).astype(np.int16)
    return x


def survives(recs, recv, kw):
    """the reference decodes the stream without crashing: tried in a child process"""
    pid = os.fork()
    if pid == 0:
        try:
            decode(recs, recv, **kw)
            os._exit(0)
        finally:
            os._exit(1)
    return os.waitpid(pid, 0)[1] == 0


def find_corrupted(wb):
    """-> [(reason, recs, trials)] and the reasons not found within TRIALS mutations: packet 3 of a clean 4-packet stream, one description hit"""
    kw = dict(WB) if wb else {}
    pcm = SP(5140, 8).reshape(4, 1280) if wb else SP(5140, 4)
    clean = encode(pcm, **kw)
    dt = L.dtypes(wb)
    emu = T.load_emu_wb() if wb else T.load_emu()
    emu.emu_dec_extract.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    h = emu.emu_dec_create(0)
    rng = np.random.default_rng(SEED + wb)
    pl0, n0, n1 = clean[3]
    found, ext = {}, np.zeros(2, dt["ext"])
    for t in range(1, TRIALS + 1):
        pl = bytearray(pl0)
        lo, hi = (0, n0 - n1) if rng.random() < 0.5 else (n0 - n1, n0 - 8)     # inside one description
        kind = rng.integers(0, 3)
        if kind == 0:
            for _ in range(rng.integers(1, 4)):
                pl[rng.integers(lo, hi)] = rng.integers(0, 256)
        elif kind == 1:
            a = rng.integers(lo, hi)
            for i in range(a, min(hi, a + int(rng.integers(1, 9)))):
                pl[i] = rng.integers(0, 256)
        else:
            pl[rng.integers(lo, hi)] ^= 1 << rng.integers(0, 8)
        buf = np.zeros(1100, np.uint8)
        buf[:n0] = np.frombuffer(bytes(pl), np.uint8)
        emu.emu_dec_extract(h, buf.ctypes.data, n0, n1, 4, ext.ctypes.data, 0)
        why = L.usable_rule(2, 0, 4, ext[0], ext[1])
        if why and why > 0 and why not in found:
            recs = clean[:3] + [(bytes(pl), n0, n1)]
            if survives(recs, np.full(4, 3, np.uint8), kw):
                found[why] = (recs, t)
        if len(found) == 5:
            break
    emu.emu_dec_destroy(h)
    missing = [L.REASONS[r] for r in (L.FS_BAD, L.ERROR, L.NARROW, L.AMBIGUOUS, L.STRUCTURE) if r not in found]
    return [(r, found[r][0], found[r][1]) for r in sorted(found)], missing, kw


def write(name, streams, wb):
    out, notes = {}, []
    lostflags, sig, interp = set(), set(), set()
    burst = lead = md1 = md2 = cng = usable = clean_desc = 0
    k = 0

    def add(title, recs, recv, kw, corrupted=-1, reason=0):
        nonlocal k, burst, lead, md1, md2, cng, usable, clean_desc
        P_ = len(recs)
        pcm, ret, ext, meta, state = decode(recs, recv, **kw)
        S = max(max(n0 for _, n0, _ in recs), 1)
        bits, nbytes = np.zeros((P_, S), np.uint8), np.zeros((P_, 2), np.int16)
        for p, (pl, n0, n1) in enumerate(recs):
            bits[p, :n0] = np.frombuffer(pl[:n0], np.uint8)
            nbytes[p] = (n0, n1)
        ms = kw.get("ms", 40)
        prm = np.array([kw.get("samplerate", 16000), kw.get("rate", 13600), kw.get("md", 0), kw.get("joint", 0), kw.get("dtx", 0), ms, P_, corrupted, reason], np.int32)
        for f, v in dict(params=prm, bits=bits, nbytes=nbytes, recv=recv, pcm=pcm, ret=ret, ext=ext.view(np.uint8).reshape(P_, 2, -1), meta=meta,
                         state=state.view(np.uint8).reshape(P_, -1)).items():
            out["s%02d_%s" % (k, f)] = v
        notes.append("s%02d = %s" % (k, title))
        k += 1
        # what the file is for
        lf = meta[:, 0]
        lostflags.update(int(v) for v in lf)
        run = lambda a: max((len(s) for s in "".join("1" if v else "0" for v in a).split("0")), default=0)
        burst, md1, md2 = max(burst, run(lf == 1)), max(md1, run(lf == 2)), max(md2, run(lf == 3))
        lead = max(lead, int(np.argmax(lf != 1)) if (lf != 1).any() else 0)
        for p in range(1, P_):
            if lf[p] == 1 and meta[p, 2] and meta[p - 1, 2] and state[p]["cng"]["rand_seed"] != state[p - 1]["cng"]["rand_seed"]:
                cng += 1
        if corrupted < 0 and ms == 40:
            for p in range(P_):
                for kk in range(2 if lf[p] == 4 else (1 if lf[p] >= 2 else 0)):
                    clean_desc += 1
                    e = ext[p, kk]
                    sig.update(int(v) >> 1 for v in e["y"]["typeOffset"])
                    interp.update(int(v) for v in e["y"]["NLSFInterpCoef_Q2"])
                if lf[p] >= 2:
                    why = L.usable_rule(2, int(meta[p, 1]), int(lf[p]), ext[p, 0], ext[p, 1])
                    assert why == 0, (title, p, why)
                    usable += 1
        return ext, meta

    for title, x, kw, kind in streams:
        if x is None:
            x = dtx_pcm()
        recs = encode(x, **kw)
        recv = masks(len(recs), kind, 7000 + k)
        add(title, recs, recv, kw)
    found, missing, kw = find_corrupted(wb)
    for reason, recs, t in found:
        ext, meta = add("corrupted: packet 3 of synth_stream(5140), %s (trial %d of seed %d)" % (L.REASONS[reason], t, SEED + wb), recs, np.full(4, 3, np.uint8), kw, 3, reason)
        print(name, "corrupted:", L.REASONS[reason], "found after", t, "trials, seed", SEED + wb, "reference ret", int(out["s%02d_ret" % (k - 1)][3]))
    print(name, "reasons not found within %d trials:" % TRIALS, missing or "none")
    print(name, "lostflags", sorted(lostflags), "burst", burst, "lead", lead, "md1 run", md1, "md2 run", md2, "cng packets", cng, "signal types", sorted(sig),
          "interpolation", sorted(interp), "clean descriptions", clean_desc, "usable packets", usable)
    assert lostflags >= {1, 2, 3, 4} and burst >= 6 and (wb or lead >= 1) and md1 >= 6 and md2 >= 6 and cng >= 1 and sig == {0, 1} and 4 in interp and min(interp) < 4
    note = ("streams: " + "; ".join(notes) + ".  Per stream: params = (samplerate, targetRate_bps, useMDIndex, joint, dtx, framesize_ms, P, corrupted packet or -1, "
            "reason), bits / nbytes / recv as solo_batch_decode takes them, pcm / ret of AGR_Sate_Decoder_Decode, ext [P][2] rows = struct SxExtracted, "
            "meta [P] = (lostflag, moreInternalDecoderFrames before, state recorded, parameter calls, frames complete, first_frame_after_reset before), "
            "state [P] rows = struct SxDecState.  reasons found: %s.  reasons not found within %d trials: %s."
            % (", ".join(L.REASONS[r] for r, _, _ in found) or "none", TRIALS, ", ".join(missing) or "none"))
    np.savez_compressed(os.path.join(HERE, name), n_streams=np.int32(k), note=np.array(note), **out)
    print("wrote", name, os.path.getsize(os.path.join(HERE, name)), "bytes")


if __name__ == "__main__":
    write("dec_stages.npz", STREAMS, False)
    write("dec_stages_wb.npz", STREAMS_WB, True)

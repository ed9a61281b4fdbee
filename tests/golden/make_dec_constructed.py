#!/usr/bin/env python3
"""Makes tests/golden/dec_constructed.npz (16 kHz API rate) and dec_constructed_wb.npz (32 kHz): CONSTRUCTED descriptions for the two branches of
the decoder's record rule that the searched fixtures (make_dec_stages.py) have no input for -- `narrow` (a pulse above 127 or more than seven LSB
planes, sx_decode_pulses) and `structure` (two usable records whose termination symbols are not "more frames, last frame", sx_extracted_usable)
-- and for the continuation of a call in the previous packet's range-coder buffers on clean data.

A case is a stream of 4 packets of synth_stream(5140) / 128 encoded by the compiled reference (a level at which PCM and state
compress: 59 cases of 4 packets then fit the size of the largest committed fixture; louder streams, whose frames are voiced, and longer ones
do not -- the voiced symbols are covered by the writer self-check over dec_stages*.npz).  Packet 1 has one or both
descriptions written again by
the host emulation's description writer (tests/emu/solo_emu.cpp: emu_write_desc) from that packet's OWN symbols, as the reference's taps hold
them, with one stated change: a pulse, the LSB planes of one block, the termination symbols, the number of frames.  Two clean packets follow.
Every payload is well-formed range-coder data with consistent lengths.  The expected values are the compiled reference's, recorded exactly as
make_dec_stages.py records them (its decode() is used): same per-stream keys, and on top of them
  family   `narrow` / `structure`, name = the case
  wdesc    [2] description 1 / 2 of packet params[7] was rewritten;  wnf [2] frames written;  wterm [2][3] termination symbol after each frame
  wsyms    [2][3] SxFrameSyms handed to the writer (bytes);  wpulses [2][3][F] int16;  wplanes [2][3][F / 16] LSB planes of every block
  wreason  [2] what the extraction must say of that description: 0 usable, SX_UNUSABLE_*
params[7] is the rewritten packet, params[8] what the rule must say of it: 0 (the records are taken), NARROW, STRUCTURE, or a description's own
reason.  For narrow and structure both follow from the change; for the two cases whose second frame is read over the bytes behind a one-frame
description, params[8] and wreason are what the host emulation's extraction says (pinned here, the same is asked of the GPU).

A case is kept only if the reference's -O2 build, its -O3 build and the tap build agree on PCM and return code of every packet, tried in a child
process first; a case that is dropped is named in the `note` with the reason.  The families asserted here are counted again from the files by
tests/test_dec_constructed.py.  Needs oracle/_ref (`make -C oracle ref taps`); runs only where the reference sources are.  The files hold data only
and are reproduced byte for byte."""
import os
import sys
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE]
import make_dec_stages as M
R, T, L = M.R, M.T, M.L

PK, P = 1, 4                # the rewritten packet, packets per stream (the files' size: see the module docstring)
QUIET = 128                  # synth_stream(5140) is divided by this
BLOCK, AT = 2, 5            # the block of 16 and the sample inside it that carry a narrow case's change
# (name, pulse or None, LSB planes or None = the fewest, per-description reason)
NARROW = [("q=127", 127, None, 0), ("7 planes", None, 7, 0), ("q=+128", 128, None, L.NARROW), ("q=-128", -128, None, L.NARROW),
          ("q=255", 255, None, L.NARROW), ("q=-1000", -1000, None, L.NARROW), ("8 planes", None, 8, L.NARROW), ("10 planes", None, 10, L.NARROW)]
DISAGREE = [(0, 0), (1, 1), (1, 2), (2, 0)]


def cases():
    """-> [(family, name, {description: (frames, terms, (frame, pulse, planes) or None)}, {packet: receive mask}, use_md_index, rule, {description: reason})]
    rule / reason None: what the emulation's extraction gives"""
    out = []
    for name, q, planes, why in NARROW:
        # frame 0 of description 1 (2 stays clean), frame 1 of description 2 (1 stays clean), and both: frame 1 of 1 and frame 0 of 2
        for where in ({0: 0}, {1: 1}, {0: 1, 1: 0}):
            out.append(("narrow", "%s in %s" % (name, " and ".join("frame %d of description %d" % (f, d + 1) for d, f in where.items())),
                        {d: (2, (1, 0), (f, q, planes)) for d, f in where.items()}, {}, 0, why, {d: why for d in where}))
    # two complete frames: frame 0 leaves bytes, frame 1 none, so the rule asks for nothing but "frame 0 announces more frames"
    rule2 = lambda t: 0 if t[0] == 1 else L.STRUCTURE
    for t0 in range(4):
        for t1 in range(4):
            out.append(("structure", "(%d,%d) in both" % (t0, t1), {0: (2, (t0, t1), None), 1: (2, (t0, t1), None)}, {}, 0, rule2((t0, t1)), {0: 0, 1: 0}))
    for t in DISAGREE:      # ONE FrameTermination, the last description's, and nBytesLeft[0]
        out.append(("structure", "(%d,%d) in description 1, (1,0) in 2" % t, {0: (2, t, None)}, {}, 0, 0, {0: 0}))
        out.append(("structure", "(1,0) in description 1, (%d,%d) in 2" % t, {1: (2, t, None)}, {}, 0, rule2(t), {1: 0}))
    for t in ((0, 0), (1, 1)):
        for mask in (1, 2):
            out.append(("structure", "(%d,%d) in both, description %d received" % (t + (mask,)), {0: (2, t, None), 1: (2, t, None)}, {PK: mask}, 0, rule2(t), {0: 0, 1: 0}))
    three = {0: (3, (1, 1, 0), None), 1: (3, (1, 1, 0), None)}
    out.append(("structure", "(1,1,0) three frames in both, next packet complete", three, {}, 0, L.STRUCTURE, {0: 0, 1: 0}))
    out.append(("structure", "(1,1,0) three frames in both, next packet description 1 only", three, {PK + 1: 1}, 0, L.STRUCTURE, {0: 0, 1: 0}))
    # description 2's registers are stale from packet 0's records when packet 2 goes on in the old buffers: the rebuild, on clean data
    out.append(("structure", "(1,1,0) three frames, description 1 received, next packet description 1 only", three, {PK: 1, PK + 1: 1}, 0, L.STRUCTURE, {0: 0, 1: 0}))
    out.append(("structure", "(1,1,0) three frames, description 2 received, next packet description 2 only", three, {PK: 2, PK + 1: 2}, 0, L.STRUCTURE, {0: 0, 1: 0}))
    out.append(("structure", "(1) one frame announcing more with nothing behind it, in both", {0: (1, (1,), None), 1: (1, (1,), None)}, {}, 0, None, {0: None, 1: None}))
    out.append(("structure", "(0) one frame, the last, in both", {0: (1, (0,), None), 1: (1, (0,), None)}, {}, 0, None, {0: None, 1: None}))
    out.append(("structure", "(0,0) in both, useMDIndex = 1", {0: (2, (0, 0), None), 1: (2, (0, 0), None)}, {}, 1, L.STRUCTURE, {0: 0, 1: 0}))
    return out


def plain(kind, recs, recv, md=0, joint=0, samplerate=16000, ms=40, **_):
    """PCM and return codes of an untapped build of the reference"""
    d = R.RefDecoder(kind, joint=joint, samplerate=samplerate, use_md_index=md, framesize_ms=ms)
    pcm, ret = np.zeros((len(recs), d.packet_samples), np.int16), np.zeros(len(recs), np.int32)
    for p, (pl, n0, n1) in enumerate(recs):
        off, a0, a1, lostflag = L.map_record(n0, n1, int(recv[p]), M.hb_bytes(joint, ms))
        pcm[p], ret[p] = d.decode(pl[off:off + a0] if lostflag != 1 else b"", a0, a1, lostflag)
    d.close()
    return pcm, ret


def agree(recs, recv, kw):
    """None, or why the case is dropped: decoded in a child process first, then by the three builds"""
    pid = os.fork()
    if pid == 0:
        try:
            M.decode(recs, recv, wide=True, **kw)
            plain("fix", recs, recv, **kw)
            plain("fix_O3", recs, recv, **kw)
            os._exit(0)
        except BaseException:
            import traceback
            traceback.print_exc()
        finally:
            os._exit(1)
    if os.waitpid(pid, 0)[1] != 0:
        return "the reference does not survive it"
    pcm, ret = M.decode(recs, recv, wide=True, **kw)[:2]
    for kind in ("fix", "fix_O3"):
        pcm2, ret2 = plain(kind, recs, recv, **kw)
        if not np.array_equal(ret, ret2):
            return "return codes of the tap build and %s differ" % kind
        if not np.array_equal(pcm, pcm2):
            return "PCM of the tap build and %s differs" % kind
    return None


def write(name, wb):
    dt = L.dtypes(wb)
    F = dt["F"]
    emu = L.writer(T.load_emu_wb() if wb else T.load_emu())
    emu.emu_dec_extract.argtypes = [M.C.c_void_p, M.C.c_void_p, M.C.c_int, M.C.c_int, M.C.c_int, M.C.c_void_p, M.C.c_int]
    base = {}
    for md in (0, 1):
        kw = dict(M.WB, md=md) if wb else dict(md=md)
        pcm = M.SP(5140, 2 * P).reshape(P, 1280) // QUIET if wb else M.SP(5140, P) // QUIET
        clean = M.encode(pcm, **kw)
        ext = M.decode(clean, np.full(P, 3, np.uint8), **kw)[2]
        assert ext[PK]["usable"].all()
        base[md] = (kw, clean, ext[PK])
    hbb = M.hb_bytes(0, 40)
    out, notes, dropped, kept = {}, [], [], []
    k = 0
    for family, title, spec, masks, md, rule, reasons in cases():
        kw, clean, e = base[md]
        pl, n0, n1 = clean[PK]
        parts = [pl[:n0 - n1], pl[n0 - n1:n0 - hbb]]
        w = dict(wdesc=np.zeros(2, np.int32), wnf=np.zeros(2, np.int32), wterm=np.full((2, 3), -1, np.int32), wsyms=np.zeros((2, 3), dt["syms"]),
                 wpulses=np.zeros((2, 3, F), np.int16), wplanes=np.zeros((2, 3, F // 16), np.int8), wreason=np.zeros(2, np.int32))
        for d, (nf, term, change) in spec.items():
            syms = e[d]["y"][[0, 1, 1]].copy()              # (a third frame repeats the second one's symbols)
            pulses = e[d]["pulses"][[0, 1, 1]].astype(np.int32)
            if change and change[1] is not None:
                pulses[change[0], BLOCK * 16 + AT] = change[1]
            planes = L.min_planes(emu, pulses)
            if change and change[2] is not None:
                assert np.abs(pulses[change[0], BLOCK * 16:BLOCK * 16 + 16]).max() <= 127 and planes[change[0], BLOCK] <= change[2]
                planes[change[0], BLOCK] = change[2]
            for f in range(nf):
                syms[f]["FrameTermination"] = term[f]
            parts[d] = L.write_desc(emu, md, syms, pulses, planes, term)
            assert parts[d] is not None, title
            w["wdesc"][d], w["wnf"][d], w["wterm"][d, :nf], w["wsyms"][d, :nf] = 1, nf, term, syms[:nf]
            w["wpulses"][d, :nf], w["wplanes"][d, :nf] = pulses[:nf], planes[:nf]
        recs = list(clean)
        recs[PK] = (parts[0] + parts[1] + pl[n0 - hbb:n0], len(parts[0]) + len(parts[1]) + hbb, len(parts[1]) + hbb)
        recv = np.full(P, 3, np.uint8)
        for p, m in masks.items():
            recv[p] = m
        why = agree(recs, recv, kw)
        if why:
            dropped.append("%s: %s (%s)" % (family, title, why))
            continue
        off, a0, a1, lf = L.map_record(recs[PK][1], recs[PK][2], int(recv[PK]), hbb)
        got = np.zeros(2, dt["ext"])
        buf = np.zeros(2200, np.uint8)
        buf[:a0] = np.frombuffer(recs[PK][0][off:off + a0], np.uint8)
        h = emu.emu_dec_create(md)
        emu.emu_dec_extract(h, buf.ctypes.data, a0, a1, lf, got.ctypes.data, 0)
        emu.emu_dec_destroy(h)
        slot = lambda d: d - (1 if lf == 3 else 0)           # description -> the slot it is handed over in (-1 / 2: not received)
        for d in spec:
            pinned = int(got[slot(d)]["pad_"][0]) if 0 <= slot(d) < (2 if lf == 4 else 1) else 0
            w["wreason"][d] = pinned if reasons[d] is None else reasons[d]
        if rule is None:
            rule = L.usable_rule(2, 0, lf, got[0], got[1])
        pcm, ret, ext, meta, state = M.decode(recs, recv, wide=True, **kw)
        S = max(n for _, n, _ in recs)
        bits, nbytes = np.zeros((P, S), np.uint8), np.zeros((P, 2), np.int16)
        for p, (b, a, c) in enumerate(recs):
            bits[p, :a] = np.frombuffer(b[:a], np.uint8)
            nbytes[p] = (a, c)
        prm = np.array([kw.get("samplerate", 16000), kw.get("rate", 13600), md, 0, 0, 40, P, PK, rule], np.int32)
        w["wsyms"] = w["wsyms"].view(np.uint8).reshape(2, 3, -1)
        for f, v in dict(params=prm, bits=bits, nbytes=nbytes, recv=recv, pcm=pcm, ret=ret, ext=ext.view(np.uint8).reshape(P, 2, -1), meta=meta,
                         state=state.view(np.uint8).reshape(P, -1), family=np.array(family), name=np.array(title), **w).items():
            out["s%02d_%s" % (k, f)] = v
        notes.append("s%02d = %s: %s -> %s, reference returns %s" % (k, family, title, L.REASONS.get(rule, rule), [int(v) for v in ret[PK:]]))
        kept.append((family, title, rule, meta))
        k += 1
    fam = lambda f, r: sum(1 for a, _, b, _ in kept if a == f and b == r)
    print(name, "kept", k, "dropped", dropped or "none", "narrow usable / narrow", fam("narrow", 0), fam("narrow", L.NARROW),
          "structure taken / structure", fam("structure", 0), fam("structure", L.STRUCTURE))
    titles = " | ".join(t for _, t, _, _ in kept) + " | " + " | ".join(dropped)
    for name_, q, planes, why in NARROW:
        assert titles.count(name_ + " in frame") == 3, name_
    for t0 in range(4):
        for t1 in range(4):
            assert "(%d,%d) in both" % (t0, t1) in titles
    for t in DISAGREE:
        assert "(%d,%d) in description 1, (1,0) in 2" % t in titles and "(1,0) in description 1, (%d,%d) in 2" % t in titles
    for s in ("description 1 received", "description 2 received", "three frames in both, next packet complete", "next packet description 1 only",
              "announcing more with nothing behind it", "one frame, the last", "useMDIndex = 1"):
        assert s in titles, s
    assert fam("narrow", 0) >= 1 and fam("narrow", L.NARROW) >= 1 and fam("structure", 0) >= 1 and fam("structure", L.STRUCTURE) >= 1
    assert any(meta[PK + 1, 1] == 1 and meta[PK + 1, 0] == 4 for _, t, _, meta in kept) and any(meta[PK + 1, 1] == 1 and meta[PK + 1, 0] == 2 for _, t, _, meta in kept)
    note = ("cases: " + "; ".join(notes) + ".  dropped: " + ("; ".join(dropped) or "none") + ".  Per stream: the keys of dec_stages.npz (params[7] = the rewritten "
            "packet, params[8] = what the rule says of it), family, name, wdesc / wnf / wterm / wsyms / wpulses / wplanes / wreason = what the writer was handed "
            "per description and what the extraction must say of it (make_dec_constructed.py).")
    np.savez_compressed(os.path.join(HERE, name), n_streams=np.int32(k), note=np.array(note), **out)
    print("wrote", name, os.path.getsize(os.path.join(HERE, name)), "bytes")


if __name__ == "__main__":
    write("dec_constructed.npz", False)
    write("dec_constructed_wb.npz", True)

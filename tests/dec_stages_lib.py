"""Layouts and data plumbing shared by tests/test_dec_stages.py and tests/golden/make_dec_stages.py: numpy structured dtypes of the decoder's
hand-over and state records (solo_amd/csrc/solo_dec.h), the conversion of the flat int32 tap records of oracle/ref_taps_dec.c into them, the
record mapping of the batched API (sx_dec_map_record, solo_dec_kernels.h) and the rule of sx_extracted_usable.  No codec arithmetic."""
import functools

import numpy as np

# SxExtracted::pad_[0] (solo_dec.h: SX_UNUSABLE_*); STRUCTURE is the test's own name for "both records usable, but frame 0 / frame 1 announce
# another number of frames than the ordinary packet" (sx_extracted_usable)
REASONS = {0: "usable", 1: "length", 2: "fs_bad", 3: "coder error", 4: "narrow", 5: "ambiguous", 6: "structure"}
LENGTH, FS_BAD, ERROR, NARROW, AMBIGUOUS, STRUCTURE = 1, 2, 3, 4, 5, 6
# offsets inside a tap record of SKP_Silk_decode_parameters (oracle/ref_taps_dec.c)
DREC_INTS, DREC_SYMS, DREC_PULSES, DREC_CTL, DREC_A = 512, 8, 96, 416, 454


def _i4(names, shape=None):
    return [(n, "<i4") if shape is None else (n, "<i4", shape) for n in names]


@functools.lru_cache(None)
def dtypes(wb):
    """-> dict of the C layouts at the 8 kHz (wb False) / 16 kHz internal rate"""
    lpc, stages, F = (16, 10, 320) if wb else (10, 6, 160)
    syms = np.dtype(_i4(("fs_bad", "MDIndex", "typeOffset")) + _i4(("GainsIndices",), (4,)) + _i4(("DeltaGainIndices",)) + _i4(("NLSFIndices",), (stages,))
                    + _i4(("NLSFInterpCoef_Q2",)) + _i4(("NLSF_Q15",), (lpc,)) + _i4(("lagIx", "conIx", "PERIndex")) + _i4(("LTPIx",), (4,))
                    + _i4(("LTPscaleIx", "Seed", "RateLevelIndex", "vadFlag", "FrameTermination", "left", "error", "bufferLength")))
    ctl = np.dtype(_i4(("pitchL", "Gains_Q16"), (4,)) + _i4(("DeltaGains_Q16", "Seed")) + [("LTPCoef_Q14", "<i2", (20,))]
                   + _i4(("LTP_scale_Q14", "PERIndex", "RateLevelIndex", "QuantOffsetType", "sigtype", "MDIndex", "NLSFInterpCoef_Q2")))
    ext = [("usable", "<i4"), ("pad_", "<i4", (3,)), ("y", syms, (2,)), ("pulses", "i1", (2, F)), ("have_A", "<i4"), ("have_hb", "<i4"),
           ("A_final", "<i2", (2, 16)), ("A_interp1", "<i2", (16,)), ("hb_lsp", "<i4", (2, 8)), ("hb_lpc", "<i2", (2, 8)), ("hb_gain", "<i2", (2, 4)),
           ("ctl", ctl, (2,)), ("lastGain", "<i4", (2,))]
    size = np.dtype(ext).itemsize
    if size % 16:                                           # alignas(16)
        ext.append(("tail_pad_", "u1", (16 - size % 16,)))
    ext = np.dtype(ext)
    desc = np.dtype(_i4(("LastGainIndex",)) + _i4(("prevNLSF_Q15",), (lpc,)) + _i4(("typeOffsetPrev", "prevDeltaGainIndex", "rc_bufferLength", "rc_bufferIx", "rc_error"))
                    + [("rc_base_Q32", "<u4"), ("rc_range_Q16", "<u4"), ("rc_tail", "<u4"), ("rc_stale", "<i4")])
    plc = np.dtype([("pitchL_Q8", "<i4"), ("LTPCoef_Q14", "<i2", (5,)), ("prevLPC_Q12", "<i2", (lpc,)), ("last_frame_lost", "<i4"), ("rand_seed", "<i4"),
                    ("randScale_Q14", "<i2"), ("prevLTP_scale_Q14", "<i2"), ("conc_energy", "<i4"), ("conc_energy_shift", "<i4"), ("prevGain_Q16", "<i4", (4,)),
                    ("fs_kHz", "<i4")], align=True)
    cng = np.dtype([("exc_buf_Q10", "<i4", (F,)), ("smth_NLSF_Q15", "<i4", (lpc,)), ("synth_state", "<i4", (lpc,)), ("smth_Gain_Q16", "<i4"), ("rand_seed", "<i4"),
                    ("fs_kHz", "<i4")])
    state = np.dtype([("md", desc, (2,)), ("prev_inv_gain_Q16", "<i4"), ("sLTP_Q16", "<i4", (2 * F,)), ("sLPC_Q14", "<i4", (16,)), ("exc_Q10", "<i4", (F,)),
                      ("outBuf", "<i2", (2 * F,))] + _i4(("lagPrev", "first_frame_after_reset", "nFramesDecoded", "moreInternalDecoderFrames", "FrameTermination",
                                                         "vadFlag", "lossCnt", "prev_sigtype", "nBytesLeft0", "started")) + [("HPState", "<i4", (2,)), ("cng", cng), ("plc", plc)]
                     + _i4(("hb_lossCnt", "hb_first", "hb_joint", "fpp")) + [("HB_prev_NLSFq", "<i4", (8,)), ("HB_synth_state", "<i4", (8,)), ("HB_prev_Gain", "<i4"),
                                                                            ("qmf_lo_hist", "<i2", (32,)), ("qmf_hi_hist", "<i2", (32,)), ("last_error", "<i4"),
                                                                            ("dbg", "<i4", (8,))], align=True)
    return dict(syms=syms, ctl=ctl, ext=ext, state=state, lpc=lpc, stages=stages, F=F)


def leaves(dt, prefix=()):
    """the scalar / array leaf fields of a structured dtype in memory order: [(path, base dtype, element count)]"""
    out = []
    for n in dt.names:
        f = dt.fields[n][0]
        base, shape = f.subdtype if f.subdtype else (f, ())
        cnt = int(np.prod(shape)) if shape else 1
        if base.names:
            for k in range(cnt):
                out += leaves(base, prefix + ((n, k if shape else None),))
        else:
            out.append((prefix + ((n, None),), base, cnt))
    return out


def unflatten(flat, dt, skip=()):
    """flat int32 values, one per element of every leaf of `dt` in memory order (leaf names in `skip`: none in `flat`, left zero) -> one record"""
    rec = np.zeros((), dt)
    i = 0
    for path, base, cnt in leaves(dt):
        if path[-1][0] in skip:
            continue
        v = rec
        for n, k in path[:-1]:
            v = v[n] if k is None else v[n][k]
        v[path[-1][0]] = np.asarray(flat[i:i + cnt]).reshape(v[path[-1][0]].shape).astype(base)
        i += cnt
    return rec, i


def name_at(dt, off):
    """name of the field of a record of type `dt` that holds byte `off`"""
    for n in dt.names:
        f, o = dt.fields[n][:2]
        if o <= off < o + f.itemsize:
            off -= o
            if f.subdtype:
                f, shape = f.subdtype
                n += "".join("[%d]" % k for k in np.unravel_index(off // f.itemsize, shape))
                off %= f.itemsize
            return n + ("." + name_at(f, off) if f.names else "")
    return "(padding)"


def span(mask, dt, *path):
    """mask[..., bytes of field path] = True; a path element is a field name or (field name, index tuple)"""
    off, size = 0, dt.itemsize
    for el in path:
        n, k = el if isinstance(el, tuple) else (el, None)
        f, o = dt.fields[n][:2]
        off += o
        if f.subdtype:
            base, shape = f.subdtype
            if k is not None:                                # (leading indices are enough: the rest of the array is spanned)
                full = tuple(k) + (0,) * (len(shape) - len(k))
                off += int(np.ravel_multi_index(full, shape)) * base.itemsize
                size = int(np.prod(shape[len(k):], dtype=np.int64)) * base.itemsize
                dt = base
                continue
        dt, size = f, f.itemsize
    mask[..., off:off + size] = True


def padding_mask(dt):
    """True for the bytes of a record of type `dt` that belong to no leaf field"""
    m = np.ones(dt.itemsize, bool)

    def walk(d, off):
        for n in d.names:
            f, o = d.fields[n][:2]
            base, shape = f.subdtype if f.subdtype else (f, ())
            for k in range(int(np.prod(shape)) if shape else 1):
                if base.names:
                    walk(base, off + o + k * base.itemsize)
                else:
                    m[off + o + k * base.itemsize:off + o + (k + 1) * base.itemsize] = False
    walk(dt, 0)
    return m


def map_record(n0, n1, recv, hbb):
    """sx_dec_map_record (solo_amd/csrc/solo_dec_kernels.h) for records that lie inside their slot: (nBytes0, nBytes1, recv mask, high-band bytes
    of the packet) -> (offset of the bytes handed over, nBytes0, nBytes1, lostflag) of the reference's calling convention"""
    m = 0 if n0 <= 0 else recv & 3
    if m == 3:
        r = (0, n0, n1, 4)
    elif m == 1:
        r = (0, n0 - n1, 0, 2)
    elif m == 2:
        r = (n0 - n1, n1, 0, 3)
    else:
        r = (0, n0 if n0 > 0 else 16, n1 if n0 > 0 else 0, 1)
    if (r[3] == 2 and r[1] <= 0) or (r[3] == 3 and r[1] <= hbb):
        r = (0, 16, 0, 1)
    return r


def desc_spans(a0, a1, lostflag, hbb):
    """sx_desc_span (solo_dec.h): where the description slots of a record handed over as (nBytes0, nBytes1, lostflag) lie inside the bytes handed
    over -> [(offset, length)] per slot in use"""
    if lostflag < 2:
        return []
    nb0 = a0 if lostflag == 2 else a0 - hbb
    nb1 = a1 - hbb if a1 else 0
    return [(0, nb0 - nb1), (nb0 - nb1, nb1)][:2 if lostflag == 4 else 1]


def writer(lib):
    """the description writer of the host emulation (tests/emu/solo_emu.cpp: emu_write_desc, emu_min_planes) with its argument types set"""
    import ctypes as C
    lib.emu_write_desc.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.emu_min_planes.argtypes = [C.c_void_p]
    return lib


def min_planes(lib, pulses):
    """pulses [..., F] of any width -> the fewest LSB planes the encoder gives every block of 16 [..., F / 16]"""
    q = np.ascontiguousarray(pulses, np.int32).reshape(-1, 16)
    out = np.array([lib.emu_min_planes(q[i].ctypes.data) for i in range(len(q))], np.int32)
    return out.reshape(np.shape(pulses)[:-1] + (np.shape(pulses)[-1] // 16,))


def write_desc(lib, use_md_index, syms, pulses, planes, term):
    """syms [n] of dtypes()["syms"], pulses [n][F], planes [n][F / 16], term [n] -> the description's bytes, or None where the writer refuses"""
    import ctypes as C
    n = len(term)
    syms, pulses = np.ascontiguousarray(syms[:n]), np.ascontiguousarray(pulses[:n], np.int32)
    planes, term = np.ascontiguousarray(planes[:n], np.int32), np.ascontiguousarray(term, np.int32)
    assert len(syms) == n and pulses.shape == (n, planes.shape[1] * 16)
    out, err = np.zeros(1100, np.uint8), C.c_int(0)
    nb = lib.emu_write_desc(n, use_md_index, syms.ctypes.data, pulses.ctypes.data, planes.ctypes.data, term.ctypes.data, out.ctypes.data, out.size, C.byref(err))
    return bytes(out[:nb]) if nb > 0 else None


def usable_rule(fpp, more_before, lostflag, e0, e1):
    """sx_extracted_usable on the packet's two records -> 0 (the records are taken) or the reason they are not (a description's own, or STRUCTURE);
    None: the packet has no description at all (lost)"""
    if lostflag < 2:
        return None
    if fpp != 2:
        return -1                                           # 20 ms packets never take records
    if more_before:
        return -2                                           # the call goes on in the previous packet's buffers
    ndesc = 2 if lostflag == 4 else 1
    for e in (e0, e1)[:ndesc]:
        if not int(e["usable"]):
            return int(e["pad_"][0]) or -3
    last = (e0, e1)[ndesc - 1]
    more0 = int(e0["y"][0]["left"]) > 0 and int(last["y"][0]["FrameTermination"]) == 1
    more1 = int(e0["y"][1]["left"]) > 0 and int(last["y"][1]["FrameTermination"]) == 1
    return 0 if more0 and not more1 else STRUCTURE

"""The encoder's analysis stage (A) and coding stage (C) ALONE against what the compiled reference hands from stage to stage, and the three stage
probes chained.  tests/golden/enc_stages.npz (16 kHz API rate) and enc_stages_wb.npz (32 kHz) hold, per stream and packet, the reference's input
PCM, the arguments of its SKP_Silk_NSQ_del_dec calls in the layout of SxNsqIn, the coded indices in the layout of SxFrameIdx, the QMF's high band,
the quantiser's outputs and the payload (tests/golden/make_enc_stages.py, oracle/ref_taps.c).

 * stage A: the fixture's PCM through the analysis stage -- sx_enc_stage_a in the host emulation, solo_enc_analysis_kernel through
   solo_debug_analysis on the GPU -- must give the reference's SxNsqIn of every frame and SxCodeIn of every packet, field by field;
 * stage C: the reference's indices, high band and quantiser output through the coding stage -- sx_enc_stage_c / solo_debug_coding -- must give
   the reference's payload bytes and byte counts, the zero counts of packets dropped by DTX included;
 * closure (GPU): solo_debug_analysis -> solo_debug_nsq_ex -> solo_debug_coding, each fed by the one before, must give the fixture's payloads:
   the probes run the kernels the pipeline runs.
With tests/test_nsq_taps.py (stage B) a broken end-to-end parity is attributed to its stage in seconds, and a hand-over field that no consumer
reads for the inputs at hand is still compared.

What is left out of the comparison (`_masks`), and nothing else:
 1. struct padding (SxNsqIn, SxFrameIdx and SxCodeIn have none);
 2. SxFrameIdx::pad_;
 3. PredCoef_Q12[k][o] for o >= the LPC order (10 at the 8 kHz internal rate): the reference leaves stack contents there, the tap zeroes them
    (so does the build's hand-over, which the byte-for-byte comparison of the chunkings relies on);
 4. the second frame's SxNsqIn and SxFrameIdx of framesize_ms = 20 packets, which hold one frame;
The masked share of every record in use is asserted to stay below 5 % of its bytes (items 2 and 3: 24 of 660 bytes of a 16 kHz SxNsqIn, 8 of 848 of
its SxCodeIn); the unused second records of item 4 are no records in use.

Fields the reference leaves UNDEFINED are compared too, against zero.  In unvoiced frames the reference never assigns PERIndex, LTPIndex[4],
LTP_scaleIndex and LTP_scale_Q14: SKP_Silk_quant_LTP_gains_FIX and SKP_Silk_LTP_scale_ctrl_FIX (SKP_Silk_LTP_scale_ctrl_FIX.c:80) run in the voiced
branch alone (SKP_Silk_find_pred_coefs_FIX.c:83, :87; unvoiced: :93-109) and the control block is an uninitialised local
(SKP_Silk_encode_frame_FIX.c:41), so it hands on what its stack held (two runs of the generator differed there).  The taps and the generator record
zero in their place, and the build's unvoiced branch (sx_find_pred_coefs, solo_enc_analysis.h) assigns zero: the records are a function of the input
alone.  Before it did, the analysis kernel published what its LDS control block held -- LTP_scale_Q14 of packet 1, frame 0 of the first
default-rate stream was 0 after one launch of all packets and 205 after launches of one packet -- which the byte-for-byte comparison of the
three chunkings below found.  (The quantiser reads LTP_scale_Q14 in unvoiced frames as well, solo_enc_nsq_row.h; only the result goes unused.)"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import solo_testlib as T

FILES = {"nb": ("enc_stages.npz", 16000), "wb": ("enc_stages_wb.npz", 32000)}
SLOT = 1024
MASK_SHARE = 0.05


def _i4(names, shape=None):
    return [(n, "<i4") if shape is None else (n, "<i4", shape) for n in names]


@functools.lru_cache(None)
def _dtypes(wb):
    L, stages = (320, 10) if wb else (160, 6)
    nsq_in = np.dtype(_i4(("sigtype", "QuantOffsetType", "NLSFInterpCoef_Q2", "Seed", "Lambda_Q10", "LTP_scale_Q14", "DeltaGains_Q16"))
                      + _i4(("pitchL", "Gains_Q16", "LF_shp_Q14", "Tilt_Q14", "HarmShapeGain_Q14"), (4,))
                      + [("PredCoef_Q12", "<i2", (2, 16)), ("LTPCoef_Q14", "<i2", (20,)), ("AR2_Q13", "<i2", (64,)), ("xfw", "<i2", (L,))])
    idx = np.dtype(_i4(("sigtype", "QuantOffsetType")) + _i4(("GainsIndices",), (4,)) + _i4(("DeltaGainsIndices",)) + _i4(("NLSFIndices",), (stages,))
                   + _i4(("NLSFInterpCoef_Q2", "lagIndex", "contourIndex", "PERIndex")) + _i4(("LTPIndex",), (4,))
                   + _i4(("LTP_scaleIndex", "Seed", "vadFlag", "inDTX", "pad_")))
    code_in = np.dtype([("idx", idx, (2,)), ("hi", "<i2", (2 * L,))])
    out = np.dtype([("Seed", "<i4"), ("r", "<i4", (L,)), ("q", "i1", (2, L + 4))])            # SxNsqOut
    ref_out = np.dtype([("Seed", "<i4"), ("q", "i1", (2, L)), ("r", "<i4", (L,))])            # the reference's record
    return nsq_in, idx, code_in, out, ref_out


def _name_at(dt, off):
    """name of the field of a record of type `dt` that holds byte `off`"""
    for n in dt.names:
        f, o = dt.fields[n][:2]
        if o <= off < o + f.itemsize:
            off -= o
            if f.subdtype:
                f, shape = f.subdtype
                n += "".join("[%d]" % k for k in np.unravel_index(off // f.itemsize, shape))
                off %= f.itemsize
            return n + ("." + _name_at(f, off) if f.names else "")
    return "(padding)"


def _span(mask, dt, *path):
    """mask[..., bytes of field path] = True; a path element is a field name or (field name, index tuple)"""
    off, size = 0, dt.itemsize
    for el in path:
        n, k = el if isinstance(el, tuple) else (el, None)
        f, o = dt.fields[n][:2]
        off += o
        if f.subdtype:
            base, shape = f.subdtype
            if k is not None:
                off += int(np.ravel_multi_index(k, shape)) * base.itemsize
                f = base
        dt, size = f, f.itemsize
    mask[..., off:off + size] = True


@functools.lru_cache(None)
def _load(rate):
    """the fixture's streams: the reference's records in the build's layouts, the masks, the init arguments"""
    name, samplerate = FILES[rate]
    wb = rate == "wb"
    z = np.load(os.path.join(T.GOLDEN, name))
    nsq_in_dt, idx_dt, code_dt, out_dt, ref_out_dt = _dtypes(wb)
    streams = []
    for k in range(int(z["n_streams"])):
        g = lambda f: z["s%02d_%s" % (k, f)]
        sr, total, md, joint, dtx, ms, P = (int(v) for v in g("params"))
        assert sr == samplerate and g("nsq_in").shape == (P, 2, nsq_in_dt.itemsize) and g("idx").shape == (P, 2, idx_dt.itemsize // 4)
        fpp = ms // 20
        cin = np.zeros(P, code_dt)
        cin["idx"] = np.ascontiguousarray(g("idx")).view(idx_dt).reshape(P, 2)
        cin["hi"][:, :g("hi").shape[1]] = g("hi")
        ref_out = np.ascontiguousarray(g("nsq_out")).view(ref_out_dt).reshape(P, 2)
        out = np.zeros((P, 2), out_dt)                                       # (as tests/test_nsq_taps.py: q rows padded by four bytes)
        out["Seed"], out["r"], out["q"][..., :ref_out["q"].shape[-1]] = ref_out["Seed"], ref_out["r"], ref_out["q"]
        nsq_in = np.ascontiguousarray(g("nsq_in")).view(nsq_in_dt).reshape(P, 2)
        m_in, m_cin = _masks(wb, fpp, cin)
        streams.append(dict(k=k, P=P, fpp=fpp, pcm=np.ascontiguousarray(g("pcm")), nsq_in=nsq_in, cin=cin, out=out, ref_out=ref_out,
                            bits=g("bits"), nbytes=g("nbytes"), nret=g("nret"), mask_in=m_in, mask_cin=m_cin, total=total, dtx=dtx,
                            init=(sr, total - (800 if joint else 1600), md, joint, dtx, fpp),          # AGR_BWE_SDK_API.c:119
                            emu=(total, md | joint << 1 | dtx << 2 | (8 if fpp == 1 else 0))))
    return streams, str(z["note"])


def _masks(wb, fpp, cin):
    """bytes left out of the comparison (module docstring): bool [P][2][sizeof SxNsqIn], bool [P][sizeof SxCodeIn]"""
    nsq_in_dt, idx_dt, code_dt = _dtypes(wb)[:3]
    P = cin.shape[0]
    m_in, m_cin = np.zeros((P, 2, nsq_in_dt.itemsize), bool), np.zeros((P, code_dt.itemsize), bool)
    for kk in range(2):
        for o in range(16 if wb else 10, 16):
            _span(m_in, nsq_in_dt, ("PredCoef_Q12", (kk, o)))
    for f in range(2):
        _span(m_cin, code_dt, ("idx", (f,)), "pad_")
    assert m_in.mean(axis=2).max() < MASK_SHARE and m_cin.mean(axis=1).max() < MASK_SHARE, (m_in.mean(axis=2).max(), m_cin.mean(axis=1).max())
    if fpp == 1:
        m_in[:, 1] = True
        _span(m_cin, code_dt, ("idx", (1,)))
    return m_in, m_cin


def _compare(got, exp, mask, dt, what, frames):
    """got / exp: records of type dt, [P] or [P][2]; on a mismatch names stream, packet, frame and every differing field of the first bad record"""
    g = np.ascontiguousarray(got).view(np.uint8).reshape(mask.shape)
    e = np.ascontiguousarray(exp).view(np.uint8).reshape(mask.shape)
    bad = (g != e) & ~mask
    if not bad.any():
        return
    first = tuple(np.argwhere(bad.reshape(bad.shape[0], -1, bad.shape[-1]).any(axis=2))[0])
    rec = bad.reshape(bad.shape[0], -1, bad.shape[-1])[first]
    fields = sorted({_name_at(dt, int(o)) for o in np.nonzero(rec)[0]})
    o = int(np.nonzero(rec)[0][0])
    raise AssertionError("%s: packet %d%s: %d differing fields, first %s%s; %d of %d records differ"
                         % (what, first[0], " frame %d" % first[1] if frames else "", len(fields), ", ".join(fields[:8]), " ..." if len(fields) > 8 else "",
                            int(bad.reshape(bad.shape[0], -1, bad.shape[-1]).any(axis=2).sum()), bad.shape[0] * (2 if frames else 1))
                         + " (byte %d: got %d, reference %d)" % (o, g.reshape(bad.shape[0], -1, bad.shape[-1])[first][o], e.reshape(bad.shape[0], -1, bad.shape[-1])[first][o]))


def _check_a(s, rate, got_in, got_cin, what):
    nsq_in_dt, _, code_dt = _dtypes(rate == "wb")[:3]
    _compare(got_in, s["nsq_in"], s["mask_in"], nsq_in_dt, "%s SxNsqIn" % what, True)
    _compare(got_cin, s["cin"], s["mask_cin"], code_dt, "%s SxCodeIn" % what, False)


def _check_c(s, bits, nbytes, status, what):
    assert status == 0, (what, "status", status)
    assert np.array_equal(nbytes, s["nbytes"]), (what, "byte counts differ, first packet", int(np.nonzero((nbytes != s["nbytes"]).any(axis=1))[0][0]))
    for p in range(s["P"]):
        n = int(s["nret"][p])            # (a packet dropped by DTX: counts 0, 0; the high band's bytes alone at the start of the slot)
        assert np.array_equal(bits[p, :n], s["bits"][p, :n]), (what, "payload differs, packet", p)


def _emu(rate):
    lib = T.load_emu_wb() if rate == "wb" else T.load_emu()
    lib.emu_analysis_packets.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.emu_coding_packets.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    return lib


# ---- the fixtures themselves ----
def test_fixtures_hold_what_they_are_for():
    """counted from the files alone: both signal types in at least four streams, voiced <-> unvoiced transitions inside a packet, at least eight
    packets dropped by DTX, NLSF interpolation on (factor < 4) and off (4), pulses of at least 20 in every stream at a rate clamp"""
    for rate in FILES:
        streams, note = _load(rate)
        both = vu = uv = dropped = 0
        interp, clamps = set(), []
        for s in streams:
            sig = s["cin"]["idx"]["sigtype"][:, :s["fpp"]]
            both += int((sig == 0).any() and (sig == 1).any())
            if s["fpp"] == 2:
                vu += int(((sig[:, 0] == 0) & (sig[:, 1] == 1)).sum())
                uv += int(((sig[:, 0] == 1) & (sig[:, 1] == 0)).sum())
            if s["dtx"]:
                dropped += int((s["nbytes"][:, 0] == 0).sum())
                assert ((s["nbytes"][:, 0] == 0) == (s["cin"]["idx"]["inDTX"][:, s["fpp"] - 1] != 0)).all()
            interp |= set(int(v) for v in s["cin"]["idx"]["NLSFInterpCoef_Q2"][:, :s["fpp"]].reshape(-1))
            if s["total"] in (101600, 6600):
                clamps.append(int(np.abs(s["ref_out"]["q"][:, :s["fpp"]].astype(np.int32)).max()))
        assert 4 in interp and min(interp) < 4 and vu >= 1 and uv >= 1, (rate, interp, vu, uv)
        assert clamps and min(clamps) >= 20 and "largest |q| of the clamp streams %d" % max(clamps) in note, (rate, clamps)
        if rate == "nb":
            assert both >= 4 and dropped >= 8 and len(streams) == 13, (both, dropped)
            assert sorted({s["init"][1:] for s in streams}) == sorted({(12000, 0, 0, 0, 2), (100000, 0, 0, 0, 2), (5000, 0, 0, 0, 2), (12000, 0, 0, 1, 2),
                                                                      (12800, 0, 1, 0, 2), (12000, 0, 0, 0, 1), (12000, 1, 0, 0, 2)})
        else:
            assert both >= 2 and len(streams) == 4


# ---- host emulation ----
@pytest.mark.parametrize("rate", list(FILES))
def test_emulated_analysis_stage_equals_the_reference_field_by_field(rate):
    lib = _emu(rate)
    nsq_in_dt, _, code_dt = _dtypes(rate == "wb")[:3]
    assert lib.emu_sizeof_nsq_in() == nsq_in_dt.itemsize and lib.emu_sizeof_code_in() == code_dt.itemsize
    # (chunk: the compact state goes through the stream record between launches.  EmuEnc keeps its work area, the control block included, from one
    # chunk to the next, where a kernel launch starts from whatever its LDS holds: that a record does not depend on the control block a launch
    # finds is checked on the GPU alone, by the byte-for-byte comparison of the three chunkings.)
    for s in _load(rate)[0]:
        for chunk in (0, 1, 7):
            got_in, got_cin = np.zeros((s["P"], 2), nsq_in_dt), np.zeros(s["P"], code_dt)
            assert lib.emu_analysis_packets(s["emu"][0], s["emu"][1], s["pcm"].ctypes.data, s["P"], chunk, got_in.ctypes.data, got_cin.ctypes.data) == nsq_in_dt.itemsize
            _check_a(s, rate, got_in, got_cin, "%s stream %d chunk %d" % (rate, s["k"], chunk))


@pytest.mark.parametrize("rate", list(FILES))
def test_emulated_coding_stage_equals_the_reference_payloads(rate):
    lib = _emu(rate)
    out_dt = _dtypes(rate == "wb")[3]
    assert lib.emu_sizeof_nsq_out() == out_dt.itemsize
    for s in _load(rate)[0]:
        for chunk in (0, 1, 5):
            bits, nbytes = np.zeros((s["P"], SLOT), np.uint8), np.full((s["P"], 2), -1, np.int16)
            status = lib.emu_coding_packets(s["emu"][0], s["emu"][1], s["cin"].ctypes.data, s["out"].ctypes.data, s["P"], chunk, SLOT, bits.ctypes.data,
                                            nbytes.ctypes.data)
            _check_c(s, bits, nbytes, status, "%s stream %d chunk %d" % (rate, s["k"], chunk))


# ---- the gfx950 kernels ----
def _groups(rate):
    """the fixture's streams by init arguments and length: one probe call initialises every stream alike"""
    groups = {}
    for s in _load(rate)[0]:
        groups.setdefault((s["init"], s["P"]), []).append(s)
    return groups


def _tiled_streams(lib, rate):
    """the stream count of the stage A runs: the smallest count above front_waves + 2 that is no multiple of front_waves (the launch table's
    streams per front workgroup)"""
    sizes = np.zeros(5, np.int32)
    nsq_in_dt, _, code_dt, out_dt = _dtypes(rate == "wb")[:4]
    assert lib.solo_debug_analysis(FILES[rate][1], 0, 0, 0, 0, 2, 0, 0, 0, None, None, None, sizes.ctypes.data) == nsq_in_dt.itemsize
    assert tuple(sizes[:4]) == (nsq_in_dt.itemsize, out_dt.itemsize, code_dt.itemsize, 1280 if rate == "wb" else 640), sizes
    fw = int(sizes[4])
    n = fw + 3
    while n % fw == 0:
        n += 1
    assert fw > 1 and n > fw and n % fw != 0, (fw, n)
    return n


def _gpu_a(lib, rate, init, group, P, n, chunk):
    nsq_in_dt, _, code_dt = _dtypes(rate == "wb")[:3]
    pcm = np.ascontiguousarray(np.stack([group[i % len(group)]["pcm"] for i in range(n)]))
    got_in, got_cin = np.zeros((n, P, 2), nsq_in_dt), np.zeros((n, P), code_dt)
    assert lib.solo_debug_analysis(*init, n, P, chunk, pcm.ctypes.data, got_in.ctypes.data, got_cin.ctypes.data, None) == nsq_in_dt.itemsize
    return got_in, got_cin


def _gpu_c(lib, rate, init, cin, out, chunk):
    n, P = cin.shape
    bits, nbytes, status = np.zeros((n, P, SLOT), np.uint8), np.zeros((n, P, 2), np.int16), np.full(n, -1, np.int32)
    assert lib.solo_debug_coding(*init, n, P, chunk, SLOT, cin.ctypes.data, out.ctypes.data, bits.ctypes.data, nbytes.ctypes.data, status.ctypes.data) == cin.dtype.itemsize
    return bits, nbytes, status


@pytest.mark.gpu
@pytest.mark.parametrize("rate", list(FILES))
def test_gpu_analysis_kernel_equals_the_reference_field_by_field(rate):
    """solo_enc_analysis_kernel alone; launches of all, 1 and 7 packets must leave identical records, byte for byte, and the reference's.  The
    streams of every group are tiled to a count above the launch table's front_waves that is no multiple of it.  (front_waves is the stream count
    of the PERSISTENT schedule's front workgroup.  The kernel this probe launches, like the launch-per-chunk pipeline, has one 64-lane workgroup
    per stream, so no workgroup here holds a ragged tail of streams; what the count gives is several workgroups and every fixture stream in more
    than one row of the hand-over arrays.)"""
    import solo_amd
    lib = solo_amd.load_library()
    n = _tiled_streams(lib, rate)
    for (init, P), group in _groups(rate).items():
        got = {chunk: _gpu_a(lib, rate, init, group, P, n, chunk) for chunk in (0, 1, 7)}
        for chunk in (1, 7):
            for a, b, nm in zip(got[0], got[chunk], ("SxNsqIn", "SxCodeIn")):
                d = np.nonzero(a.view(np.uint8).reshape(n, P, -1) != b.view(np.uint8).reshape(n, P, -1))
                assert d[0].size == 0, (rate, init, nm, "launches of %d packets differ from one launch: row %d packet %d byte %d" % (chunk, d[0][0], d[1][0], d[2][0]))
        for i in range(n):
            s = group[i % len(group)]
            _check_a(s, rate, got[0][0][i], got[0][1][i], "%s stream %d (row %d of %d)" % (rate, s["k"], i, n))


@pytest.mark.gpu
@pytest.mark.parametrize("rate", list(FILES))
def test_gpu_coding_kernels_equal_the_reference_payloads(rate):
    """solo_enc_coding_kernel + solo_enc_rc_kernel alone on the reference's indices, high band and quantiser output; 35 streams: the
    lane-per-description range coder's second wavefront (32 streams each) holds three"""
    import solo_amd
    lib = solo_amd.load_library()
    n = 35
    for (init, P), group in _groups(rate).items():
        cin = np.ascontiguousarray(np.stack([group[i % len(group)]["cin"] for i in range(n)]))
        out = np.ascontiguousarray(np.stack([group[i % len(group)]["out"] for i in range(n)]))
        for chunk in (0, 1, 5):
            bits, nbytes, status = _gpu_c(lib, rate, init, cin, out, chunk)
            for i in range(n):
                s = group[i % len(group)]
                _check_c(s, bits[i], nbytes[i], int(status[i]), "%s stream %d (row %d) chunk %d" % (rate, s["k"], i, chunk))


@pytest.mark.gpu
@pytest.mark.parametrize("rate", list(FILES))
def test_gpu_stage_probes_chained_give_the_fixture_payloads(rate):
    """analysis -> quantiser -> coding, each probe fed by the GPU output of the one before: the product pipeline's kernels, stage by stage"""
    import solo_amd
    lib = solo_amd.load_library()
    out_dt = _dtypes(rate == "wb")[3]
    n = _tiled_streams(lib, rate)
    for (init, P), group in _groups(rate).items():
        got_in, got_cin = _gpu_a(lib, rate, init, group, P, n, 0)
        out = np.zeros((n, P, 2), out_dt)
        assert lib.solo_debug_nsq_ex(*init, n, P, got_in.ctypes.data, out.ctypes.data) == out_dt.itemsize
        bits, nbytes, status = _gpu_c(lib, rate, init, got_cin, out, 0)
        for i in range(n):
            s = group[i % len(group)]
            _check_c(s, bits[i], nbytes[i], int(status[i]), "%s stream %d (row %d)" % (rate, s["k"], i))

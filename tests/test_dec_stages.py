"""The decoder's extraction step (X) and the decoder proper (S) ALONE against what the compiled reference holds at the same boundaries, and the
carried state after EVERY packet.  tests/golden/dec_stages.npz (16 kHz API rate) and dec_stages_wb.npz (32 kHz) hold, per stream and packet, the
payloads and receive masks, the reference's PCM and return code, the records of its SKP_Silk_decode_parameters calls packed as SxExtracted, and its
decoder / PLC / CNG / high-band state in the layout of SxDecState (tests/golden/make_dec_stages.py, oracle/ref_taps_dec.c).

 * stage X: every record of a received description -- sx_extract_desc through emu_dec_extract in the host emulation, solo_dec_extract_kernel
   through solo_debug_dec_extract on the GPU -- must equal the reference's, field by field: symbols, pulses, ctl[f], lastGain[f], and for the slot
   that carries them A_final, A_interp1, hb_lsp, hb_lpc, hb_gain with have_A / have_hb; `usable` and the reason in pad_[0] as predicted;
 * stage S: sx_decode_packet / solo_dec_synth_kernel fed (a) the reference's records, (b) the extraction's own, (c) none (the single kernel) must
   give the reference's PCM, return code and state after every packet, per packet and in one launch;
 * path: the rule of sx_extracted_usable, evaluated here from the reference's records and its moreInternalDecoderFrames, says which packets take
   the records; the emulation's counters (emu_dec_two_step_stats) and the records' reason codes must agree exactly -- a decoder that declared
   every record unusable would pass every PCM comparison (the serial fallback is exact) and fail here;
 * closure (GPU): extract probe -> synth probe gives solo_batch_decode's PCM byte for byte, also under SOLO_DEC_SPLIT=0 and under
   SOLO_DEC_CHUNK=3 SOLO_DEC_FIRST_CHUNK=2; raggedness: 67 (or 69) tiled streams whose description slots that carry bytes are no multiple of 64.

Corrupted descriptions.  The fixtures hold, per rate, one input for each of the reasons fs_bad, coder error and ambiguous, found by the generator's
bounded search (50000 mutations per rate).  NOT found, at either rate, also not within 300000 mutations: `narrow` (a pulse above 127 or more than
seven LSB planes without a coder error) and `structure` (two usable records whose frames announce another number of frames).  No input built to
fit stands in for them: these two branches stay without a known probing input, and the tests assert the reasons the fixture's note lists.  Where
the corrupted sampling-rate symbol names another rate the reference supports, the reference switches to it and returns 0; the build decodes one
internal rate and returns -12 (tools/debug/fuzz_decoder_gen.py: "other_rate"): the status is asserted, PCM and state of that last packet are not.

Constructed inputs for those two branches -- and for the continuation of a call in the previous packet's coder buffers on clean data -- are in
tests/test_dec_constructed.py (fixtures of their own, dec_constructed*.npz: descriptions written symbol by symbol by the host emulation's
description writer, expected values from the compiled reference); the searched fixtures here and NOT_FOUND stay as they are.

What is left out of the comparison, and nothing else.  Records (`_ext_mask`):
 1. struct padding (the tail of SxExtracted up to its 16-byte alignment) and pad_[1..2];
 2. ctl[1].MDIndex: the reference assigns MDIndex in a packet's first frame alone (SKP_Silk_decode_parameters.c:54-57), its control block is an
    uninitialised local of SKP_Silk_decode_frame; the build carries frame 0's value on;
 3. records that are not in use: slots without a received description, the records of a corrupted description beyond `usable` and the reason
    (the reference abandons the frame where its coder fails), and of 20 ms packets everything but frame 0's symbols and pulses.
ctl[0].NLSFInterpCoef_Q2 is NOT masked: where the reference overrode it after a reset (first_frame_after_reset), the coded symbol y[0] is expected.
Coefficient entries beyond the LPC order, A_* / hb_* of a slot with have_A / have_hb = 0, A_interp1 of a packet whose frame 1 does not interpolate
and the second high-band frame in joint mode are compared against zero (the taps and the probes zero them).  Masked: 20 of 1104 bytes at 16 kHz,
20 of 1504 at 32 kHz.  State (`_state_mask`):
 4. struct padding (two bytes in SxPLC at the 8 kHz internal rate);
 5. the build's own fields: md[].rc_tail, md[].rc_stale, started, fpp, hb_joint, last_error, dbg;
 6. md[].rc_bufferIx, rc_error, rc_base_Q32, rc_range_Q16 while the build's rc_stale is set (rc_bufferLength is compared).
98 of 3892 bytes at 16 kHz, 96 of 7200 at 32 kHz at most.  Both shares are asserted to stay below 5 %.  The state is compared from the first
received packet on: before it the reference runs at 24 kHz, and PCM alone is compared.
 7. after a packet the reference REJECTS (return code < 0) alone: outBuf[0, L), L the frame length.  The reference sets ret = 1 for "conceal"
    (SKP_Silk_decode_frame.c:138) and overwrites it with the error code (:150-154), so the concealment of :357 (`ret == 1`) never runs and :363
    copies the caller's output buffer -- OutLow, an uninitialised local of AGR_Sate_decode_process (AGR_BWE_decode_frame_FIX.c:137) -- into
    outBuf: the reference has no value there (in the generator's runs the stack still held the previous call's low band).  The reference's
    layout forces 320 of 3892 bytes (640 of 7200 at 32 kHz) on top of items 4-6: (98 + 320) / 3892 = 10.8 %, (96 + 640) / 7200 = 10.3 %; the cap
    for these records is 11 %.  Everything else of that state is compared, the fields the reference does update on that path included.

Found by these tests.  (1) A record the build left to chance: where frame 0's sampling-rate symbol names another rate, sx_extract_parameters
returned with only fs_bad, MDIndex, error and bufferLength of its SxFrameSyms assigned, and sx_extract_desc published the rest of the caller's
uninitialised copy; the records of the fs_bad stream differed between one launch and launches of 3 packets on the GPU (the byte-for-byte
comparison of the two chunkings).  The exit zeroes the record now.  No kernel reads such a record.  (2) A state field that
drifted: after a rejected packet the reference still runs the tail of SKP_Silk_decode_frame -- lagPrev = the parsed pitchL[3] (:391), the loss
flag of SKP_Silk_PLC_glue_frames, the comfort-noise update of SKP_Silk_CNG -- while sx_silk_decode_frame returned before all of it: lagPrev of
the 16 kHz coder-error stream was 55 after packet 3 where the reference holds 63, which would have shaped the next concealed or voiced frame.
The `ret < 0` exit restates these updates now."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import solo_testlib as T
import dec_stages_lib as L

FILES = {"nb": ("dec_stages.npz", 16000), "wb": ("dec_stages_wb.npz", 32000)}
MASK_SHARE = 0.05
MASK_SHARE_REJECTED = 0.11          # (98 + 320) / 3892 = 10.8 %, (96 + 640) / 7200 = 10.3 %: module docstring, item 7
NOT_FOUND = "narrow, structure"


@functools.lru_cache(None)
def _load(rate, files=None):
    """files: another pair of fixture files in the same layout (tests/test_dec_constructed.py), as a tuple of FILES' items"""
    name, samplerate = dict(files or FILES.items())[rate]
    wb = rate == "wb"
    dt = L.dtypes(wb)
    z = np.load(os.path.join(T.GOLDEN, name))
    streams = []
    for k in range(int(z["n_streams"])):
        g = lambda f: z["s%02d_%s" % (k, f)]
        sr, total, md, joint, dtx, ms, P, cpk, reason = (int(v) for v in g("params"))
        assert sr == samplerate
        ext = np.ascontiguousarray(g("ext")).view(dt["ext"]).reshape(P, 2)
        state = np.ascontiguousarray(g("state")).view(dt["state"]).reshape(P)
        fpp, hbb = ms // 20, 4 if (joint or ms == 20) else 8
        nbytes, recv, meta = g("nbytes"), g("recv"), g("meta")
        args = [L.map_record(int(nbytes[p, 0]), int(nbytes[p, 1]), int(recv[p]), hbb) for p in range(P)]
        assert [a[3] for a in args] == [int(v) for v in meta[:, 0]]
        # which path every packet takes, by the rule of sx_extracted_usable on the REFERENCE's values: 0 records, > 0 / < 0 fallback, None lost
        why = [reason if p == cpk else L.usable_rule(fpp, int(meta[p, 1]), args[p][3], ext[p, 0], ext[p, 1]) for p in range(P)]
        streams.append(dict(k=k, P=P, fpp=fpp, hbb=hbb, bits=g("bits"), nbytes=nbytes, recv=recv, pcm=g("pcm"), ret=g("ret"), ext=ext, meta=meta, state=state,
                            args=args, why=why, cpk=cpk, reason=reason, init=(sr, md, joint, fpp), emu=md | joint << 1 | (8 if fpp == 1 else 0),
                            other_rate=bool(cpk >= 0 and reason == L.FS_BAD and int(g("ret")[cpk]) == 0)))
    return streams, str(z["note"])


def _expected_ext(s, wb):
    """the reference's records as the extraction must leave them, and the bytes left out (module docstring)"""
    dt = L.dtypes(wb)["ext"]
    exp = s["ext"].copy()
    mask = np.zeros((s["P"], 2, dt.itemsize), bool)
    mask[:] = L.padding_mask(dt)
    L.span(mask, dt, ("pad_", (1,)))
    L.span(mask, dt, ("pad_", (2,)))
    L.span(mask, dt, ("ctl", (1,)), "MDIndex")
    assert mask.mean(axis=2).max() < MASK_SHARE, mask.mean(axis=2).max()
    in_use = np.zeros((s["P"], 2), bool)
    for p in range(s["P"]):
        lf = s["args"][p][3]
        ndesc = 2 if lf == 4 else (1 if lf >= 2 else 0)
        for k in range(2):
            if k >= ndesc or p == s["cpk"] or s["meta"][p, 1] or s["meta"][p, 4] == 0:
                mask[p, k] = True                                   # item 3; `usable` and the reason are asserted apart
            elif s["fpp"] == 1:
                mask[p, k] = True
                keep = np.zeros(dt.itemsize, bool)
                L.span(keep, dt, ("y", (0,)))
                L.span(keep, dt, ("pulses", (0,)))
                mask[p, k] &= ~keep
            else:
                in_use[p, k] = True
                if s["meta"][p, 5]:                                 # the reference overrode the factor after a reset: the symbol is expected
                    exp[p, k]["ctl"][0]["NLSFInterpCoef_Q2"] = exp[p, k]["y"][0]["NLSFInterpCoef_Q2"]
    return exp, mask, in_use


def _state_mask(got, wb, rejected=False):
    """rejected: the state after a packet the reference rejected (item 7 of the module docstring)"""
    dt = L.dtypes(wb)["state"]
    mask = np.zeros(got.shape + (dt.itemsize,), bool)
    mask[:] = L.padding_mask(dt)
    for k in range(2):
        for f in ("rc_tail", "rc_stale"):
            L.span(mask, dt, ("md", (k,)), f)
    for f in ("started", "fpp", "hb_joint", "last_error", "dbg"):
        L.span(mask, dt, f)
    for k in range(2):
        m = np.zeros(dt.itemsize, bool)
        for f in ("rc_bufferIx", "rc_error", "rc_base_Q32", "rc_range_Q16"):
            L.span(m, dt, ("md", (k,)), f)
        mask[got["md"]["rc_stale"][..., k] != 0] |= m
    if rejected:
        F = L.dtypes(wb)["F"]
        o = dt.fields["outBuf"][1]
        mask[..., o:o + 2 * F] = True
    assert mask.mean(axis=-1).max() < (MASK_SHARE_REJECTED if rejected else MASK_SHARE), mask.mean(axis=-1).max()
    return mask


def _diff(got, exp, mask, dt, what):
    """got / exp: records of type dt, any shape; names the first differing record and its fields"""
    g = np.ascontiguousarray(got).view(np.uint8).reshape(mask.shape)
    e = np.ascontiguousarray(exp).view(np.uint8).reshape(mask.shape)
    bad = (g != e) & ~mask
    if not bad.any():
        return
    first = tuple(np.argwhere(bad.any(axis=-1))[0])
    offs = np.nonzero(bad[first])[0]
    fields = sorted({L.name_at(dt, int(o)) for o in offs})
    o = int(offs[0])
    raise AssertionError("%s: record %s: %d differing fields, first %s%s; %d of %d records differ (byte %d: got %d, reference %d)"
                         % (what, first, len(fields), ", ".join(fields[:8]), " ..." if len(fields) > 8 else "", int(bad.any(axis=-1).sum()),
                            bad[..., 0].size, o, g[first][o], e[first][o]))


def _check_x(s, wb, got, what):
    """stage X: the records of one stream [P][2] against the reference's; usable and reason as predicted"""
    dt = L.dtypes(wb)["ext"]
    exp, mask, in_use = _expected_ext(s, wb)
    _diff(got, exp, mask, dt, what + " SxExtracted")
    for p in range(s["P"]):
        lf = s["args"][p][3]
        ndesc = 2 if lf == 4 else (1 if lf >= 2 else 0)
        for k in range(2):
            if k >= ndesc:
                assert got[p, k]["usable"] == 0, (what, p, k, "a slot without a description is usable")
        if ndesc and s["fpp"] == 2 and not s["meta"][p, 1]:
            why = L.usable_rule(2, 0, lf, got[p, 0], got[p, 1])
            assert why == s["why"][p], (what, "packet", p, "records say", L.REASONS.get(why, why), "predicted", L.REASONS.get(s["why"][p], s["why"][p]))
    return int(in_use.sum())


def _check_s(s, wb, pcm, status, state, what, per_packet=True):
    """stage S: PCM of every packet; with per_packet also return code and state after every packet, rejected ones included"""
    dt = L.dtypes(wb)["state"]
    last = s["P"] - (1 if s["other_rate"] else 0)
    for p in range(last):
        if s["ret"][p] == 0:
            assert np.array_equal(pcm[p], s["pcm"][p]), (what, "PCM differs, packet", p, "lostflag", s["args"][p][3])
    if not per_packet:
        return
    exp_status = [int(v) for v in s["ret"]]
    if s["other_rate"]:
        exp_status[-1] = -12
    assert [int(v) for v in status] == exp_status, (what, "status", [int(v) for v in status], exp_status)
    for p in range(last):
        if s["meta"][p, 2]:
            _diff(state[p], s["state"][p], _state_mask(state[p], wb, s["ret"][p] < 0), dt, "%s SxDecState after packet %d (lostflag %d)" % (what, p, s["args"][p][3]))


def _emu(rate):
    lib = T.load_emu_wb() if rate == "wb" else T.load_emu()
    lib.emu_dec_extract.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    lib.emu_dec_packet_recs.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.emu_dec_state_ptr.restype = C.c_void_p
    lib.emu_dec_state_ptr.argtypes = [C.c_void_p]
    return lib


def _packet(s, p):
    off, a0, a1, lf = s["args"][p]
    buf = np.zeros(s["bits"].shape[1] + 1100, np.uint8)
    n = 0 if lf == 1 else a0
    buf[:n] = s["bits"][p, off:off + n]
    return buf, a0, a1, lf


def _emu_extract(lib, s, wb):
    got = np.zeros((s["P"], 2), L.dtypes(wb)["ext"])
    h = lib.emu_dec_create(s["emu"])
    for p in range(s["P"]):
        buf, a0, a1, lf = _packet(s, p)
        lib.emu_dec_extract(h, buf.ctypes.data, a0, a1, lf, got[p].ctypes.data, 0)
    lib.emu_dec_destroy(h)
    return got


# ---- the fixtures themselves ----
def test_fixtures_hold_what_they_are_for():
    """counted from the files alone: every lostflag, a burst of >= 6 lost packets, leading loss (16 kHz), >= 6 packets of description 1 only and of
    description 2 only, CNG running, both signal types, NLSF interpolation on and off, every clean received packet of a two-frame stream taking the
    records by the reference's own values, one corrupted input per reason the note lists -- and the two reasons the search did not find"""
    for rate in FILES:
        streams, note = _load(rate)
        run = lambda a: max((len(v) for v in "".join("1" if x else "0" for x in a).split("0")), default=0)
        lf = [np.array([a[3] for a in s["args"]]) for s in streams]
        assert set(np.concatenate(lf)) == {1, 2, 3, 4}
        assert max(run(v == 1) for v in lf) >= 6 and max(run(v == 2) for v in lf) >= 6 and max(run(v == 3) for v in lf) >= 6
        if rate == "nb":
            assert max(int(np.argmax(v != 1)) for v in lf) >= 1 and len(streams) == 15
            assert {s["init"][1:] for s in streams} == {(0, 0, 2), (1, 0, 2), (0, 1, 2), (0, 0, 1)}
            assert any((s["nbytes"][:, 0] <= 0).any() for s in streams), "no empty record"
        cng = sum(int(s["state"][p]["cng"]["rand_seed"] != s["state"][p - 1]["cng"]["rand_seed"]) for s in streams for p in range(1, s["P"])
                  if s["args"][p][3] == 1 and s["meta"][p, 2] and s["meta"][p - 1, 2])
        clean = [s for s in streams if s["cpk"] < 0 and s["fpp"] == 2]
        sig = {int(v) >> 1 for s in clean for p in range(s["P"]) for k in range(2) if s["ext"][p, k]["usable"] for v in s["ext"][p, k]["y"]["typeOffset"]}
        interp = {int(v) for s in clean for p in range(s["P"]) for k in range(2) if s["ext"][p, k]["usable"] for v in s["ext"][p, k]["y"]["NLSFInterpCoef_Q2"]}
        assert cng >= 1 and sig == {0, 1} and 4 in interp and min(interp) < 4, (cng, sig, interp)
        for s in clean:
            assert all(w in (0, None) for w in s["why"]), (rate, s["k"], s["why"])
        assert sorted(s["reason"] for s in streams if s["cpk"] >= 0) == [L.FS_BAD, L.ERROR, L.AMBIGUOUS]
        assert "reasons not found within 50000 trials: %s." % NOT_FOUND in note


# ---- host emulation ----
@pytest.mark.parametrize("rate", list(FILES))
def test_emulated_extraction_equals_the_reference_field_by_field(rate):
    lib, wb = _emu(rate), rate == "wb"
    dt = L.dtypes(wb)
    assert (lib.emu_sizeof_extracted(), lib.emu_sizeof_frame_syms(), lib.emu_sizeof_dec_ctrl(), lib.emu_sizeof_dec_state()) == \
        (dt["ext"].itemsize, dt["syms"].itemsize, dt["ctl"].itemsize, dt["state"].itemsize)
    compared = 0
    for s in _load(rate)[0]:
        compared += _check_x(s, wb, _emu_extract(lib, s, wb), "%s stream %d" % (rate, s["k"]))
    assert compared >= (200 if rate == "nb" else 50), compared


@pytest.mark.parametrize("rate", list(FILES))
@pytest.mark.parametrize("source", ["reference", "extraction", "none"])
def test_emulated_decoder_proper_gives_the_reference_pcm_status_and_state(rate, source):
    """sx_decode_packet alone, from the reference's records / the extraction's / none: PCM, return code and SxDecState after every packet; and the
    path every packet took, from the emulation's counters against the rule evaluated on the reference's values"""
    lib, wb = _emu(rate), rate == "wb"
    dt = L.dtypes(wb)
    for s in _load(rate)[0]:
        recs = {"reference": s["ext"], "extraction": _emu_extract(lib, s, wb), "none": None}[source]
        h = lib.emu_dec_create(s["emu"])
        pcm, status, state = np.zeros_like(s["pcm"]), np.zeros(s["P"], np.int32), np.zeros(s["P"], dt["state"])
        u0, f0 = lib.emu_dec_two_step_stats(0), lib.emu_dec_two_step_stats(1)
        for p in range(s["P"]):
            buf, a0, a1, lf = _packet(s, p)
            r = np.ascontiguousarray(recs[p]) if recs is not None else None
            status[p] = lib.emu_dec_packet_recs(h, buf.ctypes.data, a0, a1, lf, r.ctypes.data if r is not None else None, pcm[p].ctypes.data)
            C.memmove(state[p:p + 1].ctypes.data, lib.emu_dec_state_ptr(h), dt["state"].itemsize)
        lib.emu_dec_destroy(h)
        what = "%s stream %d records: %s" % (rate, s["k"], source)
        _check_s(s, wb, pcm, status, state, what)
        why = list(s["why"])
        if source == "reference" and s["cpk"] >= 0:     # (the reference's own records of the corrupted packet: usable wherever it read both frames)
            why[s["cpk"]] = L.usable_rule(s["fpp"], int(s["meta"][s["cpk"], 1]), s["args"][s["cpk"]][3], s["ext"][s["cpk"], 0], s["ext"][s["cpk"], 1])
        took, fell = lib.emu_dec_two_step_stats(0) - u0, lib.emu_dec_two_step_stats(1) - f0
        if recs is None:
            assert (took, fell) == (0, 0), what
        else:
            assert took == sum(w == 0 for w in why), (what, "packets through the records", took, why)
            assert fell == sum(w is not None and w != 0 for w in why), (what, "fallback packets", fell, why)
            if s["fpp"] == 1:
                assert took == 0, what


def test_emulated_state_after_a_rejected_packet_equals_the_reference():
    """the state after a packet the reference REJECTED (return code -12: the `coder error` stream of either fixture, packet 3, lostflag 4), from
    the single-kernel path: everything but the frame of outBuf the reference fills from uninitialised memory (module docstring, item 7) -- the
    lag, the loss flag and the comfort-noise estimate it does update on that path included (sx_silk_decode_frame, `ret < 0`)"""
    for rate in FILES:
        lib, wb = _emu(rate), rate == "wb"
        dt = L.dtypes(wb)
        seen = 0
        for s in _load(rate)[0]:
            if not (s["ret"] < 0).any():
                continue
            h = lib.emu_dec_create(s["emu"])
            pcm, status, state = np.zeros_like(s["pcm"]), np.zeros(s["P"], np.int32), np.zeros(s["P"], dt["state"])
            for p in range(s["P"]):
                buf, a0, a1, lf = _packet(s, p)
                status[p] = lib.emu_dec_packet_recs(h, buf.ctypes.data, a0, a1, lf, None, pcm[p].ctypes.data)
                C.memmove(state[p:p + 1].ctypes.data, lib.emu_dec_state_ptr(h), dt["state"].itemsize)
            lib.emu_dec_destroy(h)
            _check_s(s, wb, pcm, status, state, "%s stream %d" % (rate, s["k"]))
            seen += int(sum(1 for p in range(s["P"]) if s["ret"][p] < 0 and s["meta"][p, 2]))
        assert seen >= 1, rate


# ---- the gfx950 kernels ----
def _groups(rate):
    groups = {}
    for s in _load(rate)[0]:
        groups.setdefault((s["init"], s["P"]), []).append(s)
    return groups


def _tile(group, n):
    """the group's streams tiled to n rows: bits [n][P][slot], nbytes, recv; slot = the longest payload of the fixture + 8"""
    slot = max(s["bits"].shape[1] for s in group) + 8
    P = group[0]["P"]
    bits, nbytes, recv = np.zeros((n, P, slot), np.uint8), np.zeros((n, P, 2), np.int16), np.zeros((n, P), np.uint8)
    for i in range(n):
        s = group[i % len(group)]
        bits[i, :, :s["bits"].shape[1]], nbytes[i], recv[i] = s["bits"], s["nbytes"], s["recv"]
    return bits, nbytes, recv, slot


def _rows(group):
    """67 rows, or 69 where 67 would make the description slots that carry bytes a multiple of 64; -> rows, those slots"""
    for n in (67, 69):
        slots = sum(sum({4: 2, 3: 1, 2: 1, 1: 0}[a[3]] for a in group[i % len(group)]["args"]) for i in range(n))
        if slots % 64:
            return n, slots
    raise AssertionError("no ragged row count")


def _gpu_extract(lib, rate, init, tiled, chunk):
    bits, nbytes, recv, slot = tiled
    n, P = recv.shape
    dt = L.dtypes(rate == "wb")["ext"]
    got, counts = np.zeros((n, P, 2), dt), np.full(P, -7, np.int32)
    assert lib.solo_debug_dec_extract(*init, n, P, chunk, slot, bits.ctypes.data, nbytes.ctypes.data, recv.ctypes.data, got.ctypes.data, counts.ctypes.data) == dt.itemsize
    return got, counts


def _gpu_synth(lib, rate, init, tiled, recs, chunk):
    bits, nbytes, recv, slot = tiled
    n, P = recv.shape
    dt = L.dtypes(rate == "wb")
    launches = (P + chunk - 1) // chunk if chunk else 1
    pcm = np.zeros((n, P, (1280 if rate == "wb" else 640) // 2 * init[3]), np.int16)
    status, state = np.zeros((launches, n), np.int32), np.zeros((launches, n), dt["state"])
    assert lib.solo_debug_dec_synth(*init, n, P, chunk, slot, bits.ctypes.data, nbytes.ctypes.data, recv.ctypes.data, recs.ctypes.data if recs is not None else None,
                                    pcm.ctypes.data, status.ctypes.data, state.ctypes.data, dt["state"].itemsize) == dt["ext"].itemsize
    return pcm, status, state


@pytest.mark.gpu
@pytest.mark.parametrize("rate", list(FILES))
def test_gpu_extraction_kernel_equals_the_reference_field_by_field(rate):
    """solo_dec_list_kernel + solo_dec_extract_kernel alone on 67 tiled streams: the listed slots are no multiple of 64 (the last wavefront of the
    extraction is ragged) and equal the slots that carry bytes; every tiled copy equals the reference record for record; launches of 3 packets leave
    the records of one launch"""
    import solo_amd
    lib = solo_amd.load_library()
    wb = rate == "wb"
    assert lib.solo_debug_dec_extract(FILES[rate][1], 0, 0, 2, 0, 0, 0, 0, None, None, None, None, None) == L.dtypes(wb)["ext"].itemsize
    for (init, P), group in _groups(rate).items():
        n, slots = _rows(group)
        assert slots % 64 != 0
        tiled = _tile(group, n)
        got, counts = _gpu_extract(lib, rate, init, tiled, 0)
        assert int(counts[0]) == slots, (rate, init, "listed description slots", int(counts[0]), slots)
        got3, counts3 = _gpu_extract(lib, rate, init, tiled, 3)
        assert int(counts3[:(P + 2) // 3].sum()) == slots
        assert np.array_equal(got.view(np.uint8), got3.view(np.uint8)), (rate, init, "launches of 3 packets leave other records")
        for i in range(n):
            s = group[i % len(group)]
            _check_x(s, wb, got[i], "%s stream %d (row %d of %d)" % (rate, s["k"], i, n))
            if i >= len(group):
                assert np.array_equal(got[i].view(np.uint8), got[i % len(group)].view(np.uint8)), (rate, init, "row", i, "differs from its original")


@pytest.mark.gpu
@pytest.mark.parametrize("rate", list(FILES))
def test_gpu_decoder_proper_gives_the_reference_pcm_status_and_state(rate):
    """solo_dec_synth_kernel alone from the reference's records and from the extract probe's, and the single kernel without records: launches of one
    packet give PCM, status and SxDecState after every packet; one launch gives the same PCM and the final state.  The path: a record the
    synthesis would not take says so in `usable` / pad_[0] / its frames' structure, checked against the rule on the reference's values by stage X;
    here the records handed over are the ones whose path was checked."""
    import solo_amd
    lib = solo_amd.load_library()
    wb = rate == "wb"
    dt = L.dtypes(wb)["state"]
    for (init, P), group in _groups(rate).items():
        n = len(group) + 1                                               # (one tiled copy: two workgroups see the same stream)
        tiled = _tile(group, n)
        ref = np.ascontiguousarray(np.stack([group[i % len(group)]["ext"] for i in range(n)]))
        own = _gpu_extract(lib, rate, init, tiled, 0)[0]
        for source, recs in (("reference", ref), ("extraction", own), ("none", None)):
            pcm1, status1, state1 = _gpu_synth(lib, rate, init, tiled, recs, 1)
            pcm0, status0, state0 = _gpu_synth(lib, rate, init, tiled, recs, 0)
            for i in range(n):
                s = group[i % len(group)]
                what = "%s stream %d (row %d) records: %s" % (rate, s["k"], i, source)
                # (the synthesis kernel's status word keeps the first error of the call: per packet it is the launch's own where none came before)
                st = status1[:, i].copy()
                if recs is not None:
                    first = np.nonzero(st)[0]
                    assert first.size == 0 or (st[first[0]:] == st[first[0]]).all(), (what, st)
                    if first.size:
                        st[first[0] + 1:] = s["ret"][first[0] + 1:] if not s["other_rate"] else 0
                _check_s(s, wb, pcm1[i], st, state1[:, i], what)
                _check_s(s, wb, pcm0[i], None, None, what + " one launch", per_packet=False)
                last = s["P"] - 1
                if not s["other_rate"] and s["meta"][last, 2]:
                    L_ = state0[0, i]
                    _diff(L_, s["state"][last], _state_mask(L_, wb, s["ret"][last] < 0), dt, what + " SxDecState after one launch")


@pytest.mark.gpu
@pytest.mark.parametrize("rate", list(FILES))
def test_gpu_probes_chained_give_the_pipelines_pcm(rate):
    """extract probe -> synth probe = solo_batch_decode for the same call, byte for byte; and = the single-kernel path (SOLO_DEC_SPLIT=0) and the
    chunked pipeline (SOLO_DEC_CHUNK=3 SOLO_DEC_FIRST_CHUNK=2)"""
    import torch
    import solo_amd
    lib = solo_amd.load_library()
    knobs = ({}, {"SOLO_DEC_SPLIT": "0"}, {"SOLO_DEC_CHUNK": "3", "SOLO_DEC_FIRST_CHUNK": "2"})
    for (init, P), group in _groups(rate).items():
        n = len(group) + 3
        tiled = _tile(group, n)
        bits, nbytes, recv, slot = tiled
        pcm = _gpu_synth(lib, rate, init, tiled, _gpu_extract(lib, rate, init, tiled, 0)[0], 0)[0]
        for env in knobs:
            old = {k: os.environ.get(k) for k in env}
            os.environ.update(env)
            try:
                b = solo_amd.SoloBatch(n, encoder=False, decoder=True, slot_bytes=slot, use_md_index=init[1], joint=init[2], samplerate=init[0],
                                       framesize_ms=20 * init[3])
                out, _ = b.decode(torch.from_numpy(bits).cuda(), torch.from_numpy(nbytes).cuda(), torch.from_numpy(recv).cuda())
                torch.cuda.synchronize()
            finally:
                for k, v in old.items():
                    if v is None:
                        os.environ.pop(k, None)
                    else:
                        os.environ[k] = v
            assert np.array_equal(out.cpu().numpy(), pcm), (rate, init, env, "solo_batch_decode differs from the chained probes")

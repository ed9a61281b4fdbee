"""The decoder's record rule on CONSTRUCTED descriptions: the two branches tests/test_dec_stages.py has no input for, and the continuation of a
call in the previous packet's range-coder buffers on clean data.

solo_dec_synth_kernel takes a packet's records from the extraction only when sx_extracted_usable (solo_dec.h) says the packet is an ordinary one;
everything else goes through the serial fallback with the exact history.  A record taken when it must not be gives wrong PCM for that packet and
leaves moreInternalDecoderFrames and the coder registers wrong for the packets after it.  Random corruption does not reach the branches behind
that decision (a flipped byte nearly always ends in a coder error first); a writer that codes chosen symbols does, on both sides of each boundary.

 * the writer: emu_write_desc (tests/emu/solo_emu.cpp), test infrastructure next to the host emulation.  It shares the range encoder, the shell
   coder's split and the tables with the product; the layout of a description and the pulse part (any magnitude, LSB planes as the caller
   chooses) are its own.  Self-check: fed the reference's symbols and pulses of every clean received description of every 40 ms stream of
   dec_stages.npz / dec_stages_wb.npz (useMDIndex = 1 included), the fewest planes and terminations (1, 0), it reproduces the bytes exactly.
 * the cases: tests/golden/dec_constructed.npz (16 kHz API rate) and dec_constructed_wb.npz (32 kHz), tests/golden/make_dec_constructed.py: streams
   of 4 packets from the reference encoder, packet 1 with one or both descriptions written again from its own symbols with one change, two
   clean packets behind it; PCM, return code, tapped records and SxDecState after every packet from the compiled reference (-O2, -O3 and tap
   build agree on every case).  `narrow`: |q| = 127 and 7 LSB planes (usable controls), q = +128, -128, 255, -1000, 8 and 10 planes on a block of
   small pulses (the nl > 7 branch alone), each in frame 0 of description 1, in frame 1 of description 2, and in both descriptions (frame 1 of
   description 1, frame 0 of description 2).  `structure`: all 16 termination pairs in both descriptions, the descriptions disagreeing both
   ways round, one description received, a well-formed three-frame description (1,1,0) whose third frame the NEXT call reads from the old
   buffers -- with both descriptions, and with one, where the other slot's registers are stale from the packet before and are rebuilt from
   the shadow buffer --, a frame announcing more with nothing behind it, a one-frame description, useMDIndex = 1.
 * stage X, the rule, stage S and the closure are those of tests/test_dec_stages.py, with its masks and caps and nothing else taken out.  A
   rewritten description's record says `usable` / pad_[0] as the fixture does; where usable it equals the writer's input, symbol for symbol
   and pulse for pulse, and the reference's taps wherever the reference read both frames in the ordinary order.

The FEC bookkeeping the reference updates on termination symbols 2 and 3 (no_FEC_counter, inband_FEC_offset: SKP_Silk_dec_API.c:134-148) is not
part of SxDecState: it shapes no output of this decoder (LBRR payloads are never searched); PCM and state of the packets behind are the evidence.

Found by these tests.  Rule, fallback and the rebuild of stale registers agree with the reference on every case.  One divergence in the
extraction's reason code: with byte storage sx_decode_pulses kept a pulse above 127 as its low byte; where that came out <= 0 (128, 255, 1000)
the sign bit was skipped and the symbols behind the pulses were read from the wrong place -- q = +128 in frame 1 of description 2 said `coder
error`, not `narrow` (unusable either way: no output changed).  The pulse is kept as 127 now and its sign is read (DESIGN_NOTES.md, section 5).

Not a full cross of the narrow family: each change sits in three places, not six, and the streams are 4 quiet packets (unvoiced frames), because
the files may not exceed the largest committed fixture; the voiced symbols go through the writer in the self-check."""
import ctypes as C
import os

import numpy as np
import pytest

import solo_testlib as T
import dec_stages_lib as L
import test_dec_stages as S

FILES = {"nb": ("dec_constructed.npz", 16000), "wb": ("dec_constructed_wb.npz", 32000)}
_ITEMS = tuple(FILES.items())
EXTRA = ("family", "name", "wdesc", "wnf", "wterm", "wsyms", "wpulses", "wplanes", "wreason")
SYMBOLS = ("MDIndex", "typeOffset", "GainsIndices", "DeltaGainIndices", "NLSFIndices", "NLSFInterpCoef_Q2", "lagIx", "conIx", "PERIndex", "LTPIx", "LTPscaleIx",
           "Seed", "RateLevelIndex", "vadFlag", "FrameTermination")


def _load(rate):
    streams, note = S._load(rate, _ITEMS)
    if "family" not in streams[0]:
        z = np.load(os.path.join(T.GOLDEN, FILES[rate][0]))
        dt = L.dtypes(rate == "wb")
        for s in streams:
            for f in EXTRA:
                s[f] = z["s%02d_%s" % (s["k"], f)]
            s["family"], s["name"] = str(s["family"]), str(s["name"])
            s["wsyms"] = np.ascontiguousarray(s["wsyms"]).view(dt["syms"]).reshape(2, 3)
    return streams, note


def _slots(s, p):
    """-> [(slot, description)] of packet p as it is handed over"""
    lf = s["args"][p][3]
    return {4: [(0, 0), (1, 1)], 3: [(0, 1)], 2: [(0, 0)], 1: []}[lf]


def _check_x(s, wb, got, what):
    """stage X for one stream: every packet but the rewritten one as tests/test_dec_stages.py checks it; the rewritten one description by description"""
    dt = L.dtypes(wb)["ext"]
    pk = s["cpk"]
    exp, mask, in_use = S._expected_ext(s, wb)
    S._diff(got, exp, mask, dt, what + " SxExtracted")
    for p in range(s["P"]):
        for k in range(len(_slots(s, p)), 2):
            assert got[p, k]["usable"] == 0, (what, p, k, "a slot without a description is usable")
        if _slots(s, p):
            why = L.usable_rule(2, int(s["meta"][p, 1]), s["args"][p][3], got[p, 0], got[p, 1])
            assert why == s["why"][p], (what, "packet", p, "records say", L.REASONS.get(why, why), "predicted", L.REASONS.get(s["why"][p], s["why"][p]))
    base = np.zeros(dt.itemsize, bool)
    base[:] = L.padding_mask(dt)
    for el in (("pad_", (1,)), ("pad_", (2,))):
        L.span(base, dt, el)
    L.span(base, dt, ("ctl", (1,)), "MDIndex")
    assert base.mean() < S.MASK_SHARE
    compared = int(in_use.sum())
    for k, d in _slots(s, pk):
        g, ref = got[pk, k], s["ext"][pk, k].copy()
        who = "%s packet %d description %d" % (what, pk, d + 1)
        if s["wdesc"][d]:
            assert (int(g["usable"]), int(g["pad_"][0])) == (int(s["wreason"][d] == 0), int(s["wreason"][d])), (who, int(g["usable"]), L.REASONS.get(int(g["pad_"][0])))
        else:
            assert (int(g["usable"]), int(g["pad_"][0])) == (1, 0), (who, "the clean partner is not usable")
        if not g["usable"]:
            continue
        if s["wdesc"][d] and s["wnf"][d] >= 2:
            for f in range(2):
                for n in SYMBOLS:
                    assert np.array_equal(g["y"][f][n], s["wsyms"][d, f][n]), (who, "frame", f, n, g["y"][f][n], s["wsyms"][d, f][n])
                assert np.array_equal(g["pulses"][f].astype(np.int32), s["wpulses"][d, f].astype(np.int32)), (who, "frame", f, "pulses")
        if ref["usable"]:
            if s["meta"][pk, 5]:
                ref["ctl"][0]["NLSFInterpCoef_Q2"] = ref["y"][0]["NLSFInterpCoef_Q2"]
            S._diff(g, ref, base, dt, who + " against the reference's taps")
            compared += 1
        else:
            assert not s["wdesc"][d] or s["why"][pk] != 0 or s["wnf"][d] != 2, (who, "a packet that is taken has no reference record")
    return compared


def _emu_run(lib, s, wb, recs):
    dt = L.dtypes(wb)
    h = lib.emu_dec_create(s["emu"])
    pcm, status, state = np.zeros_like(s["pcm"]), np.zeros(s["P"], np.int32), np.zeros(s["P"], dt["state"])
    u0, f0 = lib.emu_dec_two_step_stats(0), lib.emu_dec_two_step_stats(1)
    for p in range(s["P"]):
        buf, a0, a1, lf = S._packet(s, p)
        r = np.ascontiguousarray(recs[p]) if recs is not None else None
        status[p] = lib.emu_dec_packet_recs(h, buf.ctypes.data, a0, a1, lf, r.ctypes.data if r is not None else None, pcm[p].ctypes.data)
        C.memmove(state[p:p + 1].ctypes.data, lib.emu_dec_state_ptr(h), dt["state"].itemsize)
    lib.emu_dec_destroy(h)
    return pcm, status, state, lib.emu_dec_two_step_stats(0) - u0, lib.emu_dec_two_step_stats(1) - f0


# ---- the writer and the fixtures ----
def test_writer_reproduces_every_clean_description_of_the_stage_fixtures():
    for rate in S.FILES:
        lib = L.writer(S._emu(rate))
        n, md = 0, 0
        for s in S._load(rate)[0]:
            if s["fpp"] != 2:
                continue
            for p in range(s["P"]):
                off, a0, a1, lf = s["args"][p]
                for k, (o, ln) in enumerate(L.desc_spans(a0, a1, lf, s["hbb"])):
                    e = s["ext"][p, k]
                    if not e["usable"] or p == s["cpk"]:
                        continue
                    pulses = e["pulses"].astype(np.int32)
                    got = L.write_desc(lib, s["init"][1], e["y"], pulses, L.min_planes(lib, pulses), [1, 0])
                    assert got == bytes(s["bits"][p, off + o:off + o + ln]), (rate, "stream", s["k"], "packet", p, "slot", k)
                    n += 1
                    md += s["init"][1]
        assert n >= (200 if rate == "nb" else 50) and md >= 10, (rate, n, md)


def test_writer_refuses_what_has_no_code():
    """fewer planes than the block needs, a termination symbol outside 0..3, no frames"""
    lib = L.writer(S._emu("nb"))
    s = _load("nb")[0][0]
    y, q = s["wsyms"][0], s["wpulses"][0].astype(np.int32)
    planes = L.min_planes(lib, q)
    assert L.write_desc(lib, 0, y, q, planes, [1, 0]) is not None
    q[0, 7] = 500
    assert L.min_planes(lib, q)[0, 0] > planes[0, 0] and L.write_desc(lib, 0, y, q, planes, [1, 0]) is None
    assert L.write_desc(lib, 0, y, s["wpulses"][0].astype(np.int32), planes, [1, 4]) is None


def test_fixtures_hold_every_family():
    """counted from the files alone, from what the writer was handed (not from the cases' names)"""
    limit = os.path.getsize(os.path.join(T.GOLDEN, "synth8x25.npz"))
    for rate in FILES:
        streams, note = _load(rate)
        lib = L.writer(S._emu(rate))
        assert os.path.getsize(os.path.join(T.GOLDEN, FILES[rate][0])) <= limit
        narrow, pairs, disagree, one_recv, three, short, md = {}, set(), set(), set(), set(), set(), 0
        for s in streams:
            pk = s["cpk"]
            assert s["P"] <= 6 and 1 <= pk <= s["P"] - 3 and s["name"] in note and (s["recv"][pk + 1:] != 0).all() and s["recv"][:pk].tolist() == [3] * pk
            assert s["why"][pk - 1] == 0, "the packet before goes through the records"
            d_ = [d for d in range(2) if s["wdesc"][d]]
            if s["family"] == "narrow":
                kind = set()
                for d in d_:
                    q, pl = s["wpulses"][d, :2].astype(np.int32), s["wplanes"][d, :2].astype(np.int32)
                    more = np.argwhere(pl != L.min_planes(lib, q))          # the block whose planes the caller chose
                    if len(more):
                        assert len(more) == 1
                        f, blk = (int(v) for v in more[0])
                        assert np.abs(q[f, blk * 16:blk * 16 + 16]).max() <= 127 and np.abs(q).max() <= 127, "the planes alone"
                        kind.add((0, int(pl[f, blk])))
                    else:
                        f, i = (int(v) for v in np.unravel_index(np.abs(q).argmax(), q.shape))
                        assert np.abs(q[f, i]) >= 127 and (np.abs(np.delete(q.ravel(), f * q.shape[1] + i)) < 127).all(), "one pulse"
                        kind.add((int(q[f, i]), 0))
                    assert s["wreason"][d] == (L.NARROW if np.abs(q).max() > 127 or pl.max() > 7 else 0) and s["wterm"][d].tolist() == [1, 0, -1]
                    narrow.setdefault(min(kind), set()).add((tuple(d_), f))
                assert len(kind) == 1 and s["reason"] == max(s["wreason"][d] for d in d_)
            else:
                t = [tuple(int(v) for v in s["wterm"][d, :s["wnf"][d]]) for d in range(2)]
                md += s["init"][1]
                lf, nxt = s["args"][pk][3], s["args"][pk + 1][3]
                if max(s["wnf"]) == 3:
                    assert t[0] == t[1] == (1, 1, 0) and s["why"][pk] == L.STRUCTURE and s["why"][pk + 1] == -2 and s["meta"][pk + 1, 1] == 1
                    three.add((lf, nxt))
                elif max(s["wnf"]) == 1:
                    short.add(t[0])
                elif len(d_) == 1:
                    disagree.add((d_[0], t[d_[0]]))
                elif lf != 4:
                    one_recv.add((lf, t[0]))
                elif not s["init"][1]:
                    assert t[0] == t[1]
                    pairs.add(t[0])
                    assert s["why"][pk] == (0 if t[0][0] == 1 else L.STRUCTURE)
        assert set(narrow) == {(127, 0), (0, 7), (128, 0), (-128, 0), (255, 0), (-1000, 0), (0, 8), (0, 10)}, (rate, sorted(narrow))
        for kind, where in narrow.items():
            assert {w[0] for w in where} == {(0,), (1,), (0, 1)} and {w[1] for w in where} == {0, 1}, (rate, kind, where)
        assert pairs == {(a, b) for a in range(4) for b in range(4)}
        assert disagree >= {(d, t) for d in range(2) for t in ((0, 0), (1, 1), (1, 2), (2, 0))}
        assert one_recv >= {(lf, t) for lf in (2, 3) for t in ((0, 0), (1, 1))}
        assert three >= {(4, 4), (4, 2), (2, 2), (3, 3)} and short == {(1,), (0,)} and md >= 1
        by = lambda fam, r: sum(1 for s in streams if s["family"] == fam and s["reason"] == r)
        assert by("narrow", 0) >= 2 and by("narrow", L.NARROW) >= 6 and by("structure", 0) >= 1 and by("structure", L.STRUCTURE) >= 1
        assert "dropped: none." in note, "a dropped case is named in the note with its reason; the families above are all present"


# ---- host emulation ----
@pytest.mark.parametrize("rate", list(FILES))
def test_emulated_extraction_of_constructed_descriptions(rate):
    lib, wb = S._emu(rate), rate == "wb"
    compared = 0
    for s in _load(rate)[0]:
        compared += _check_x(s, wb, S._emu_extract(lib, s, wb), "%s stream %d (%s)" % (rate, s["k"], s["name"]))
    assert compared >= 150, compared


@pytest.mark.parametrize("rate", list(FILES))
def test_rule_takes_exactly_the_packets_it_must(rate):
    """the rule on the emulation's own records: 0 for the controls, NARROW, STRUCTURE, -2 for the packet behind a (1,1,...) one; and the emulation's
    counters: exactly those packets take the records, exactly the others fall back"""
    lib, wb = S._emu(rate), rate == "wb"
    seen = set()
    for s in _load(rate)[0]:
        got = S._emu_extract(lib, s, wb)
        why = [L.usable_rule(2, int(s["meta"][p, 1]), s["args"][p][3], got[p, 0], got[p, 1]) for p in range(s["P"])]
        assert why == s["why"] and why[s["cpk"]] == s["reason"], (rate, s["name"], why, s["why"])
        seen.update((s["family"], w) for w in why)
        took, fell = _emu_run(lib, s, wb, got)[3:]
        assert (took, fell) == (sum(w == 0 for w in why), sum(w is not None and w != 0 for w in why)), (rate, s["name"], took, fell, why)
    assert seen >= {("narrow", 0), ("narrow", L.NARROW), ("structure", 0), ("structure", L.STRUCTURE), ("structure", -2)}, seen


@pytest.mark.parametrize("rate", list(FILES))
@pytest.mark.parametrize("source", ["extraction", "none"])
def test_emulated_decoder_gives_the_reference_pcm_status_and_state(rate, source):
    lib, wb = S._emu(rate), rate == "wb"
    rejected = 0
    for s in _load(rate)[0]:
        recs = S._emu_extract(lib, s, wb) if source == "extraction" else None
        pcm, status, state = _emu_run(lib, s, wb, recs)[:3]
        S._check_s(s, wb, pcm, status, state, "%s stream %d (%s) records: %s" % (rate, s["k"], s["name"], source))
        rejected += int((s["ret"] < 0).sum())
    assert rejected >= 1         # (the continuation reads a slot whose buffer is used up: the state after a rejected packet is compared too)


# ---- the gfx950 kernels ----
def _groups(rate):
    groups = {}
    for s in _load(rate)[0]:
        groups.setdefault((s["init"], s["P"]), []).append(s)
    return groups


@pytest.mark.gpu
@pytest.mark.parametrize("rate", list(FILES))
def test_gpu_extraction_of_constructed_descriptions(rate):
    """solo_debug_dec_extract on the cases tiled to 67 (69) rows: rewritten descriptions between clean ones all over the extraction's workgroups;
    every record as in stage X, the neighbours' too (a lane's LDS byte row that ran over into the next lane's shows here and nowhere on the CPU);
    launches of all packets and of 3 packets leave byte-identical records"""
    import solo_amd
    lib = solo_amd.load_library()
    wb = rate == "wb"
    for (init, P), group in _groups(rate).items():
        n, slots = S._rows(group)
        tiled = S._tile(group, n)
        got, counts = S._gpu_extract(lib, rate, init, tiled, 0)
        assert int(counts[0]) == slots and slots % 64 != 0, (rate, init, int(counts[0]), slots)
        got3, counts3 = S._gpu_extract(lib, rate, init, tiled, 3)
        assert int(counts3[:(P + 2) // 3].sum()) == slots
        assert np.array_equal(got.view(np.uint8), got3.view(np.uint8)), (rate, init, "launches of 3 packets leave other records")
        # one launch per packet: the launch of the rewritten packet lists slot (row, description) at place 2 * row + description, so stream 0's
        # rewritten description 1 sits in the first lane of a workgroup (64 lanes, 32 at 32 kHz) and stream 31's description 2 in the last
        if len(group) > 31:
            assert group[0]["wdesc"][0] and group[31]["wdesc"][1] and (tiled[2][:32, group[0]["cpk"]] == 3).all()
        got1 = S._gpu_extract(lib, rate, init, tiled, 1)[0]
        assert np.array_equal(got.view(np.uint8), got1.view(np.uint8)), (rate, init, "launches of 1 packet leave other records")
        for i in range(n):
            s = group[i % len(group)]
            _check_x(s, wb, got[i], "%s stream %d (%s, row %d of %d)" % (rate, s["k"], s["name"], i, n))
            if i >= len(group):
                assert np.array_equal(got[i].view(np.uint8), got[i % len(group)].view(np.uint8)), (rate, init, "row", i, "differs from its original")


@pytest.mark.gpu
@pytest.mark.parametrize("rate", list(FILES))
def test_gpu_decoder_gives_the_reference_pcm_status_and_state(rate):
    """solo_debug_dec_synth from the extract probe's records, from the reference's where the fixture has them (elsewhere they say unusable: the
    fallback), and without records: PCM, status and the whole SxDecState after every packet; one launch gives the same PCM"""
    import solo_amd
    lib = solo_amd.load_library()
    wb = rate == "wb"
    for (init, P), group in _groups(rate).items():
        n = len(group) + 1
        tiled = S._tile(group, n)
        ref = np.ascontiguousarray(np.stack([group[i % len(group)]["ext"] for i in range(n)]))
        own = S._gpu_extract(lib, rate, init, tiled, 0)[0]
        for source, recs in (("extraction", own), ("reference", ref), ("none", None)):
            pcm1, status1, state1 = S._gpu_synth(lib, rate, init, tiled, recs, 1)
            pcm0 = S._gpu_synth(lib, rate, init, tiled, recs, 0)[0]
            for i in range(n):
                s = group[i % len(group)]
                what = "%s stream %d (%s, row %d) records: %s" % (rate, s["k"], s["name"], i, source)
                st = status1[:, i].copy()
                if recs is not None:        # (the synthesis kernel's status word keeps the first error of the call: tests/test_dec_stages.py)
                    first = np.nonzero(st)[0]
                    assert first.size == 0 or (st[first[0]:] == st[first[0]]).all(), (what, st)
                    if first.size:
                        st[first[0] + 1:] = s["ret"][first[0] + 1:]
                S._check_s(s, wb, pcm1[i], st, state1[:, i], what)
                S._check_s(s, wb, pcm0[i], None, None, what + " one launch", per_packet=False)


@pytest.mark.gpu
@pytest.mark.parametrize("rate", list(FILES))
def test_gpu_probes_chained_give_the_pipelines_pcm(rate):
    """extract probe -> synth probe = solo_batch_decode byte for byte: by default, under SOLO_DEC_SPLIT=0, under SOLO_DEC_CHUNK=3
    SOLO_DEC_FIRST_CHUNK=2, and with the rewritten packet as the LAST packet of a call (the continuation in the old buffers crosses a call)"""
    import torch
    import solo_amd
    lib = solo_amd.load_library()
    knobs = ({}, {"SOLO_DEC_SPLIT": "0"}, {"SOLO_DEC_CHUNK": "3", "SOLO_DEC_FIRST_CHUNK": "2"}, {"cut": "1"})
    for (init, P), group in _groups(rate).items():
        n, _ = S._rows(group)
        tiled = S._tile(group, n)
        bits, nbytes, recv, slot = tiled
        pk = group[0]["cpk"]
        assert all(s["cpk"] == pk for s in group)
        pcm = S._gpu_synth(lib, rate, init, tiled, S._gpu_extract(lib, rate, init, tiled, 0)[0], 0)[0]
        for env in knobs:
            env = dict(env)
            cut = env.pop("cut", None)
            old = {k: os.environ.get(k) for k in env}
            os.environ.update(env)
            try:
                b = solo_amd.SoloBatch(n, encoder=False, decoder=True, slot_bytes=slot, use_md_index=init[1], joint=init[2], samplerate=init[0],
                                       framesize_ms=20 * init[3])
                outs = []
                for lo, hi in (((0, pk + 1), (pk + 1, P)) if cut else ((0, P),)):
                    g = lambda a: torch.from_numpy(np.ascontiguousarray(a[:, lo:hi])).cuda()
                    outs.append(b.decode(g(bits), g(nbytes), g(recv))[0].cpu().numpy())
                torch.cuda.synchronize()
            finally:
                for k, v in old.items():
                    if v is None:
                        os.environ.pop(k, None)
                    else:
                        os.environ[k] = v
            assert np.array_equal(np.concatenate(outs, axis=1), pcm), (rate, init, env, cut, "solo_batch_decode differs from the chained probes")

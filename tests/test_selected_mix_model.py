"""Shared listener mixes from a given selection without a GPU (solo_mix_selected): the passes of solo_amd/csrc/solo_mix_selected.h are
compiled for the host by this test (tests/selected_mix_host.cpp, through tests/host_build.py) and compared bit for bit with the
independent model of tests/selected_mix_model.py -- PCM, lists, source table, room_nsel, energies, counts, and the fill behind the counts.
Two identities tie the call to the host forms of solo_mix_shared and solo_mix, and one family runs through a stand-alone build of the
same file under the address and undefined-behaviour sanitisers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from host_build import FLAGS, host_lib, source
from selected_mix_model import heard, model_mix_selected, selected_case
from shared_mix_model import shared_case

FILL = dict(pcm_spk=0x1234, spk_list=-7001, spk_rows=-7002, pcm_room=0x4321, room_list=-7003, source=-7004, room_nsel=0xA5, energy=-77)
DTYPE = dict(pcm_spk=np.int16, spk_list=np.int32, spk_rows=np.int32, pcm_room=np.int16, room_list=np.int32, source=np.int32, room_nsel=np.uint8,
             energy=np.int64)
OPTIONAL = ("spk_rows", "room_nsel", "energy")
FILL_C = 0x5A5A5A5A
COUNT = ("rows", "rooms", "speakers", "shared", "clipped", "selected", "silent")
SRC = source("selected_mix")


@pytest.fixture(scope="module")
def host():
    lib = host_lib("selected_mix")
    V, I = C.c_void_p, C.c_int
    lib.emu_mix_selected.argtypes = [V, I, I, I, V, I] + [V] * 13
    lib.emu_mix_shared.argtypes = [V, I, I, I, V, I, V, I, V, V, V, V, V, V, V, V, V, V, V]
    lib.emu_mix.argtypes = [V, I, I, I, V, I, V, I, V, V, V, V]
    lib.emu_mixsel_scratch_bytes.restype = C.c_longlong
    return lib


def aligned(shape, dtype, fill=0):
    """an array whose first byte is 16-byte aligned (the interface's rule for PCM)"""
    nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
    raw = np.zeros(nbytes + 16, np.uint8)
    off = (-raw.ctypes.data) % 16
    a = raw[off:off + nbytes].view(dtype).reshape(shape)
    a[...] = fill
    return a


def ptr(a):
    return a.ctypes.data if a is not None else None


def buffers(n, n_rooms, P, L):
    shapes = dict(pcm_spk=(n, P, L), spk_list=(n,), spk_rows=(n,), pcm_room=(n_rooms, P, L), room_list=(n_rooms,), source=(n,), room_nsel=(n_rooms, P),
                  energy=(n, P))
    b = {k: aligned(s, DTYPE[k], FILL[k]) for k, s in shapes.items()}
    b["count"] = np.full(8, FILL_C, np.int32)
    return b


def count_of(cnt):
    c = dict(rows=int(cnt[0]), rooms=int(cnt[1]), speakers=int(cnt[2]), shared=int(cnt[3]), clipped=int(cnt[4:6].view(np.int64)[0]),
             selected=int(cnt[6]), silent=int(cnt[7]))
    assert tuple(c) == COUNT
    return c


def run_sel(host, pcm, room, n_rooms, gain, sel, keep, slots, drop=()):
    n, P, L = pcm.shape
    x = aligned(pcm.shape, np.int16)
    x[...] = pcm
    b = buffers(n, n_rooms, P, L)
    room = np.ascontiguousarray(room, np.int32)
    sel = np.ascontiguousarray(sel, np.uint8)
    a = {k: (None if k in drop else v) for k, v in b.items()}
    ret = host.emu_mix_selected(ptr(x), n, P, L, ptr(room), n_rooms, ptr(gain), ptr(sel), ptr(keep), ptr(slots), ptr(a["pcm_spk"]), ptr(a["spk_list"]),
                                ptr(a["spk_rows"]), ptr(a["pcm_room"]), ptr(a["room_list"]), ptr(a["source"]), ptr(a["room_nsel"]), ptr(a["energy"]),
                                ptr(a["count"]))
    return ret, b


def sel_want(pcm, room, n_rooms, gain, sel, keep, slots):
    n, P, L = pcm.shape
    return model_mix_selected(pcm, room, n_rooms, sel, gain, keep, slots, fill={k: v for k, v in buffers(n, n_rooms, P, L).items() if k != "count"})


def same(got, want, skip=()):
    """every array against the model (which started from the same fill: what must not be written is compared too)"""
    for k in FILL:
        if k in skip:
            assert (got[k] == FILL[k]).all(), k
        else:
            bad = np.argwhere(got[k] != want[k])
            assert len(bad) == 0, (k, bad[:6].tolist())


def untouched(b, count_from=1):
    return all((b[k] == FILL[k]).all() for k in FILL) and (b["count"][count_from:] == FILL_C).all()


def family_has_everything(pcm, room, gain, n_rooms, sel, keep, slots, marks, want):
    """the generator's family holds what the interface names (P packets)"""
    n, P, L = pcm.shape
    on = (sel != 0) & (room >= 0)[:, None]
    per = lambda name: on[marks[name]].sum(axis=0)                               # selected members of a room, per packet
    size = lambda name: len(marks[name])
    # rooms with 0, 1, some and all members selected
    assert (per("nobody") == 0).all() and (per("moving") == 1).all() and (per("steady") == 1).all()
    assert 1 < per("some")[0] < size("some") and (per("everyone") == size("everyone")).all() and (per("one") == 1).all() and size("one") == 1
    assert per("big")[0] == min(size("big") - 1, 64)
    # rows in no room with sel set, kept rows that are never selected, a kept row in no room
    loose = marks["loose"]
    assert (room[loose] == -1).all() and sel[loose].any() and keep[loose].any()
    never = (room >= 0) & (keep != 0) & ~on.any(axis=1)
    assert never[marks["some"]].any() and never[marks["big"]].any() and never[marks["kept"]].all()
    if P >= 3:                                                                   # a selection that changes from packet to packet
        assert len({tuple(on[marks["moving"], p]) for p in range(P)}) == P and per("some").tolist()[:3] == [3, 1, 0]
        assert per("big").tolist()[:3] == [min(size("big") - 1, 64), 5, 1]
    g_on = set(gain[on.any(axis=1)].tolist())
    assert {0, -5, 32767} <= g_on                                                # selected rows with gains zero, negative and 32767
    assert set(np.unique(sel)) > {0, 1}                                          # any non-zero byte selects
    assert (np.diff(slots) > 1).any()
    c = want["count"]
    assert c["clipped"] > 0 and c["silent"] > 0 and 0 < c["shared"] < c["rooms"] and 0 < c["speakers"] < c["rows"] == (room >= 0).sum()
    assert c["selected"] == int(on.sum()) < int((sel != 0).sum())
    shared = want["room_list"][:c["shared"]].tolist()
    room_of = lambda name: int(room[marks[name][0]])
    assert room_of("nobody") in shared and room_of("some") in shared and room_of("big") in shared and room_of("moving") in shared
    assert room_of("one") not in shared and room_of("everyone") not in shared and room_of("kept") not in shared
    # the kept room: speakers who hear zeros
    for i in marks["kept"]:
        assert 0 <= want["source"][i] < n and not want["pcm_spk"][want["source"][i]].any()
    j = shared.index(room_of("nobody"))
    assert not want["pcm_room"][j].any() and not want["room_nsel"][j].any()


@pytest.mark.parametrize("L,P", [(320, 1), (320, 3), (640, 1), (640, 3), (1280, 1), (1280, 3)])
def test_host_mix_selected_against_model(host, L, P):
    case = selected_case(500 + L + P, P, L)
    pcm, room, gain, n_rooms, sel, keep, slots, marks = case
    want = sel_want(pcm, room, n_rooms, gain, sel, keep, slots)
    family_has_everything(*case, want)
    ret, got = run_sel(host, pcm, room, n_rooms, gain, sel, keep, slots)
    assert ret == 0 and count_of(got["count"]) == want["count"], (count_of(got["count"]), want["count"])
    same(got, want)
    # gains, keep, slots, d_spk_rows, d_room_nsel and d_energy NULL
    want = sel_want(pcm, room, n_rooms, None, sel, None, None)
    ret, got = run_sel(host, pcm, room, n_rooms, None, sel, None, None, drop=OPTIONAL)
    assert ret == 0 and count_of(got["count"]) == want["count"], (count_of(got["count"]), want["count"])
    same(got, want, skip=OPTIONAL)
    ns = want["count"]["speakers"]
    assert np.array_equal(got["spk_list"][:ns], want["spk_rows"][:ns])


def test_scratch_formula(host):
    # seven words per row, the picks and their counts per row and packet (the header's "8 bytes per row and packet + 28 per row")
    assert host.emu_mixsel_scratch_bytes(1000, 7) == 8 * 1000 * 7 + 28 * 1000 and host.emu_mixsel_count_size() == 32


def test_mix_selected_host_refusals(host):
    P, L = 2, 320
    pcm, room, gain, n_rooms, sel, keep, slots, _ = selected_case(12, P, L, big=12)
    n = len(room)
    x = aligned(pcm.shape, np.int16)
    x[...] = pcm
    b = buffers(n + 1, n_rooms + 1, P, L)
    room = np.ascontiguousarray(room, np.int32)
    row = P * L * 2

    def call(pin=ptr(x), n=n, P=P, L=L, room=ptr(room), n_rooms=n_rooms, sel=ptr(sel), spk=ptr(b["pcm_spk"]), spk_list=ptr(b["spk_list"]),
             proom=ptr(b["pcm_room"]), room_list=ptr(b["room_list"]), source=ptr(b["source"]), count=ptr(b["count"])):
        return host.emu_mix_selected(pin, n, P, L, room, n_rooms, ptr(gain), sel, ptr(keep), ptr(slots), spk, spk_list, ptr(b["spk_rows"]), proom,
                                     room_list, source, ptr(b["room_nsel"]), ptr(b["energy"]), count)

    # what solo_mix_shared refuses (it has no max_speakers here)
    assert call(pin=None) == -1 and call(room=None) == -1
    assert call(n=0) == -1 and call(n=-3) == -1 and call(P=0) == -1 and call(n_rooms=0) == -1 and call(n_rooms=n + 1) == -1
    assert call(n=2, P=2 ** 30, n_rooms=1) == -1                                       # n * n_packets = 2^31
    assert call(L=0) == -1 and call(L=1288) == -1 and call(L=324) == -1                # the packet geometry
    assert call(pin=ptr(x) + 2) == -1 and call(spk=ptr(b["pcm_spk"]) + 8) == -1 and call(proom=ptr(b["pcm_room"]) + 4) == -1      # not 16-byte aligned
    # a NULL selection
    assert call(sel=None) == -1
    # required outputs
    assert call(spk=None) == -1 and call(spk_list=None) == -1 and call(proom=None) == -1 and call(room_list=None) == -1
    assert call(source=None) == -1 and call(count=None) == -1
    # overlaps: each output with the input, and the outputs with each other (by one row at either end)
    assert call(spk=ptr(x)) == -1 and call(proom=ptr(x)) == -1 and call(proom=ptr(b["pcm_spk"])) == -1
    assert call(spk=ptr(x) + (n - 1) * row) == -1 and call(pin=ptr(b["pcm_spk"]) + (n - 1) * row) == -1
    assert call(proom=ptr(x) + (n - 1) * row) == -1 and call(pin=ptr(b["pcm_room"]) + (n_rooms - 1) * row) == -1
    assert call(proom=ptr(b["pcm_spk"]) + (n - 1) * row) == -1 and call(spk=ptr(b["pcm_room"]) + (n_rooms - 1) * row) == -1
    assert untouched(b, 0)
    assert call() == 0 and b["count"][0] == (room >= 0).sum()


@pytest.mark.parametrize("what", ["room_low", "room_high", "room_max", "slots_negative", "slots_equal", "slots_falling", "sel_65", "sel_all_70"])
def test_mix_selected_device_refusals(host, what):
    """in each, nothing but rows = -1 is written (pre-filled buffers); 65 selected in one (room, packet) of a room of 70 among them"""
    P, L = 2, 320
    pcm, room, gain, n_rooms, sel, keep, slots, marks = selected_case(13, P, L)
    room, slots, sel = room.copy(), slots.copy(), sel.copy()
    if what.startswith("room"):
        room[5] = dict(room_low=-2, room_high=n_rooms, room_max=2 ** 31 - 1)[what]
    elif what == "slots_negative":
        slots[0] = -1
    elif what.startswith("slots"):
        slots[9] = slots[8] if what == "slots_equal" else slots[8] - 1
    else:
        big = marks["big"]
        assert len(big) == 70 and (sel[big, 1] != 0).sum() == 5
        if what == "sel_65":                                                     # packet 1 of the room: 65 of 70
            sel[big[:65], 1] = 1
            sel[big[65:], 1] = 0
            assert (sel[big, 1] != 0).sum() == 65 and (sel[big, 0] != 0).sum() == 64
        else:
            sel[big, 1] = 3
    ret, got = run_sel(host, pcm, room, n_rooms, gain, sel, keep, slots)
    assert ret == -2 and got["count"][0] == -1 and untouched(got)
    assert model_mix_selected(pcm, room, n_rooms, sel, gain, keep, slots)["count"]["rows"] == -1


def test_sixty_four_selected_are_accepted(host):
    """the bound itself: 64 of 70 in every packet"""
    P, L = 2, 320
    pcm, room, gain, n_rooms, sel, keep, slots, marks = selected_case(14, P, L)
    sel = sel.copy()
    sel[marks["big"][:64], 1] = 1
    sel[marks["big"][64:], 1] = 0
    want = sel_want(pcm, room, n_rooms, gain, sel, keep, slots)
    ret, got = run_sel(host, pcm, room, n_rooms, gain, sel, keep, slots)
    assert ret == 0 and count_of(got["count"]) == want["count"]
    same(got, want)


# ---- identities against the host forms of the existing calls ----------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 3])
def test_selection_of_mix_shared_gives_mix_shared(host, K):
    """with sel := d_mixed of a solo_mix_shared run on the same arguments, every common output is byte-equal to that run's"""
    P, L = 3, 640
    pcm, room, gain, n_rooms, keep, slots, _ = shared_case(600 + K, P, L, K)
    n = len(room)
    x = aligned(pcm.shape, np.int16)
    x[...] = pcm
    room = np.ascontiguousarray(room, np.int32)
    sb = buffers(n, n_rooms, P, L)
    mixed = np.full((n, P), 0xA5, np.uint8)
    scount = np.full(6, FILL_C, np.int32)
    assert host.emu_mix_shared(ptr(x), n, P, L, ptr(room), n_rooms, ptr(gain), K, ptr(keep), ptr(slots), ptr(sb["pcm_spk"]), ptr(sb["spk_list"]),
                               ptr(sb["spk_rows"]), ptr(sb["pcm_room"]), ptr(sb["room_list"]), ptr(sb["source"]), ptr(sb["energy"]), ptr(mixed),
                               ptr(scount)) == 0
    sel = np.where(room[:, None] >= 0, mixed, 0).astype(np.uint8)                # (rows in no room keep the fill: not a selection)
    ret, got = run_sel(host, pcm, room, n_rooms, gain, sel, keep, slots)
    assert ret == 0
    c = count_of(got["count"])
    ns, nr = int(scount[2]), int(scount[3])
    assert [c[k] for k in COUNT[:4]] == scount[:4].tolist() and c["clipped"] == int(scount[4:6].view(np.int64)[0]) and ns > 0 and nr > 0
    for k, m in (("pcm_spk", ns), ("spk_list", ns), ("spk_rows", ns), ("pcm_room", nr), ("room_list", nr), ("source", n)):
        assert got[k][:m].tobytes() == sb[k][:m].tobytes(), k
    assert np.array_equal(got["energy"], sb["energy"])


@pytest.mark.parametrize("L", [320, 640, 1280])
def test_everybody_hears_what_solo_mix_gives(host, L):
    """at P = 1 every row hears through `source` what solo_mix gives it with the gains sel ? gain : 0 and max_speakers = 64"""
    pcm, room, gain, n_rooms, sel, keep, slots, _ = selected_case(700 + L, 1, L)
    n = len(room)
    ret, got = run_sel(host, pcm, room, n_rooms, gain, sel, keep, slots)
    assert ret == 0
    x = aligned(pcm.shape, np.int16)
    x[...] = pcm
    room = np.ascontiguousarray(room, np.int32)
    masked = np.where(sel[:, 0] != 0, gain, 0).astype(np.int16)
    out = aligned(pcm.shape, np.int16, 0x77)
    mcount = np.zeros(4, np.int32)
    assert host.emu_mix(ptr(x), n, 1, L, ptr(room), n_rooms, ptr(masked), 64, ptr(out), None, None, ptr(mcount)) == 0
    inroom = room >= 0
    assert np.array_equal(heard(got, n)[inroom], out[inroom])


# ---- the same source as a stand-alone program under the sanitisers -----------------------------------------------------------------------
def test_stand_alone_build_under_the_sanitisers(tmp_path):
    """tests/selected_mix_host.cpp with its own main, -fsanitize=address,undefined: one family in through a file, every output back through
    a file and against the model; any report of a sanitiser ends the program with a non-zero status"""
    exe = str(tmp_path / "selected_mix_asan")
    flags = [f for f in FLAGS if f not in ("-shared", "-fPIC", "-O2")] + ["-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                                                                         "-fno-sanitize-recover=all", "-DSELECTED_MIX_MAIN"]
    cxx = os.environ.get("CXX", "g++")
    if os.path.basename(cxx).startswith("g++"):                                  # the runtimes inside the program: nothing has to load ahead of it
        flags += ["-static-libasan", "-static-libubsan"]
    subprocess.check_call([cxx] + flags + [SRC, "-o", exe])
    P, L = 3, 640
    pcm, room, gain, n_rooms, sel, keep, slots, _ = selected_case(800, P, L)
    n = len(room)
    for optional in (1, 0):
        fin, fout = str(tmp_path / ("in%d.bin" % optional)), str(tmp_path / ("out%d.bin" % optional))
        with open(fin, "wb") as f:
            f.write(np.array([n, P, L, n_rooms, optional, optional, optional, optional], np.int32).tobytes())
            for a, dt in ((pcm, np.int16), (room, np.int32), (gain, np.int16), (sel, np.uint8), (keep, np.uint8), (slots, np.int32)):
                f.write(np.ascontiguousarray(a, dt).tobytes())
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        r = subprocess.run([exe, fin, fout], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        raw = open(fout, "rb").read()
        want = model_mix_selected(pcm, room, n_rooms, sel, *((gain, keep, slots) if optional else (None, None, None)))
        assert np.frombuffer(raw[:4], np.int32)[0] == 0
        at = 4
        for k, shape in (("pcm_spk", (n, P, L)), ("spk_list", (n,)), ("spk_rows", (n,)), ("pcm_room", (n_rooms, P, L)), ("room_list", (n_rooms,)),
                         ("source", (n,)), ("room_nsel", (n_rooms, P)), ("energy", (n, P))):
            size = int(np.prod(shape)) * np.dtype(DTYPE[k]).itemsize
            got = np.frombuffer(raw[at:at + size], DTYPE[k]).reshape(shape)
            at += size
            if not optional and k in OPTIONAL:
                assert not got.any(), k
            else:
                assert np.array_equal(got, want[k]), k
        assert count_of(np.frombuffer(raw[at:at + 32], np.int32)) == want["count"] and at + 32 == len(raw)

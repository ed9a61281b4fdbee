"""solo_vad / solo_vad_select (include/solo_mi355x.h): the symbols exist, the Python layer knows them, and every host refusal the header
lists returns "refused" from the very checks the entry points run (solo_amd/csrc/solo_vad.h, through the host build of
tests/vad_host.cpp: no GPU call is made here)."""
import ctypes as C
import os

import numpy as np
import pytest

import solo_amd
import solo_testlib as T
from test_vad_model import build_host

SYMBOLS = ("solo_vad_create", "solo_vad_destroy", "solo_vad_reset", "solo_vad_reset_rows", "solo_vad_get_state", "solo_vad_set_state", "solo_vad",
           "solo_vad_select")


@pytest.fixture(scope="module")
def host():
    return build_host()


def test_symbols_and_layouts(host):
    if not os.path.exists(solo_amd.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = C.CDLL(solo_amd.LIB_PATH)
    for s in SYMBOLS:
        assert s in solo_amd.ABI_SYMBOLS and hasattr(lib, s), s
    assert C.sizeof(solo_amd.solo_vad_count_t) == host.emu_vad_count_size() == 16
    assert C.sizeof(solo_amd.solo_vad_select_params_t) == host.emu_vad_params_size() == 20
    assert solo_amd.VAD_STATE_BYTES == host.emu_vad_state_bytes() == 128
    hdr = open(os.path.join(T.ROOT, "include", "solo_mi355x.h")).read()
    assert "#define SOLO_VAD_STATE_BYTES 128" in hdr
    assert hasattr(solo_amd, "Vad") and solo_amd.Vad.COUNT == ("rows", "rooms", "selected", "changes")


def test_frame_lengths(host):
    for f in (-320, 0, 80, 159, 161, 240, 319, 321, 480, 640):
        assert host.emu_vad_frame_ok(f) == 0, f
    assert host.emu_vad_frame_ok(160) == 1 and host.emu_vad_frame_ok(320) == 1


def test_solo_vad_refusals(host):
    buf = np.zeros(64, dtype=np.int16)
    a = (buf.ctypes.data + 15) & ~15                        # (never dereferenced: the checks look at addresses only)
    sa, cnt, rows = a + 4096, a + 8192, a + 12288
    ok = lambda frame=320, n_rows=8, rows=None, n=8, pcm=a, P=1, Ls=640, sa=sa, count=None: host.emu_vad_call_ok(frame, n_rows, rows, n, pcm, P, Ls, sa, count)
    assert ok() == 1 and ok(rows=rows, count=cnt, n=3) == 1 and ok(count=cnt) == 1
    assert ok(pcm=None) == 0 and ok(sa=None) == 0
    assert ok(rows=rows) == 0                               # d_count is required with d_rows
    for n in (0, -1, 9):
        assert ok(n=n) == 0
    assert ok(P=0) == 0 and ok(P=-1) == 0
    for frame, good, bad in ((320, (320, 640, 960, 1280, 1600, 1920), (0, -320, 160, 319, 321, 480, 2240, 3200)),
                             (160, (160, 320, 480, 640, 1920), (0, -160, 80, 159, 161, 240, 2080))):
        for Ls in good:
            assert ok(frame=frame, Ls=Ls) == 1, (frame, Ls)
        for Ls in bad:
            assert ok(frame=frame, Ls=Ls) == 0, (frame, Ls)
    assert ok(frame=240, Ls=240) == 0
    for off in (2, 4, 8):
        assert ok(pcm=a + off) == 0
    assert ok(n_rows=1 << 20, n=1 << 20, P=4, Ls=640) == 0          # 2^31 samples and more
    assert ok(n_rows=1 << 20, n=1 << 20, P=3, Ls=640) == 1
    arr = lambda v: np.array(v, dtype=np.int32).ctypes.data
    assert host.emu_vad_list_ok(arr([0, 2]), 2, 4) == 1 and host.emu_vad_list_ok(arr([2, 0]), 2, 4) == 1
    assert host.emu_vad_list_ok(arr([0, 0]), 2, 4) == 0 and host.emu_vad_list_ok(arr([0, 4]), 2, 4) == 0 and host.emu_vad_list_ok(arr([-1]), 1, 4) == 0
    assert host.emu_vad_list_ok(arr([0, 1, 2, 3, 0]), 5, 4) == 0 and host.emu_vad_list_ok(None, 1, 4) == 0 and host.emu_vad_list_ok(arr([0]), 0, 4) == 0


def test_solo_vad_select_refusals(host):
    a = 4096                                                # (addresses are only compared with NULL)
    prm = lambda **kw: np.array([kw.get(k, d) for k, d in (("max_speakers", 3), ("on", 128), ("off", 64), ("hang", 5), ("stick", 6))], dtype=np.int32)

    def ok(n_rows=8, n=8, sa=a, level=a, P=1, frames=2, room=a, n_rooms=4, p=prm(), sel=a, count=a):
        return host.emu_vsel_call_ok(n_rows, n, sa, level, P, frames, room, n_rooms, None if p is None else p.ctypes.data, sel, count)
    assert ok() == 1
    for name in ("sa", "level", "room", "p", "sel", "count"):
        assert ok(**{name: None}) == 0, name
    for n in (0, -1, 9):
        assert ok(n=n) == 0
    assert ok(P=0) == 0 and ok(frames=0) == 0 and ok(n_rooms=0) == 0 and ok(n_rooms=9) == 0 and ok(n_rooms=8) == 1
    assert ok(n_rows=1 << 20, n=1 << 20, P=1 << 10, frames=2) == 0 and ok(n_rows=1 << 20, n=4, n_rooms=1 << 20, P=1 << 11) == 0
    for good in (dict(max_speakers=1), dict(max_speakers=64), dict(on=255, off=255), dict(on=0, off=0), dict(hang=0), dict(hang=1000), dict(stick=0),
                 dict(stick=127)):
        assert ok(p=prm(**good)) == 1, good
    for bad in (dict(max_speakers=0), dict(max_speakers=65), dict(max_speakers=-1), dict(on=256), dict(off=-1), dict(on=63, off=64), dict(hang=-1),
                dict(hang=1001), dict(stick=-1), dict(stick=128)):
        assert ok(p=prm(**bad)) == 0, bad

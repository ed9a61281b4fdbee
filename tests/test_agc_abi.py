"""solo_agc (include/solo_mi355x.h): the symbols exist, the Python layer knows them, and every host refusal the header lists returns
"refused" from the very checks the entry point runs (solo_amd/csrc/solo_agc.h, through the host build of tests/agc_host.cpp: no GPU
call is made here)."""
import ctypes as C
import os

import numpy as np
import pytest

import agc_lib as L
import agc_model as M
import solo_amd
import solo_testlib as T

SYMBOLS = ("solo_agc_create", "solo_agc_destroy", "solo_agc_reset", "solo_agc_reset_rows", "solo_agc_get_state", "solo_agc_set_state", "solo_agc")


@pytest.fixture(scope="module")
def host():
    return L.build_host()


def test_symbols_and_layouts(host):
    if not os.path.exists(solo_amd.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = C.CDLL(solo_amd.LIB_PATH)
    for s in SYMBOLS:
        assert s in solo_amd.ABI_SYMBOLS and hasattr(lib, s), s
    assert C.sizeof(solo_amd.solo_agc_count_t) == host.emu_agc_count_size() == 16
    assert C.sizeof(solo_amd.solo_agc_params_t) == host.emu_agc_params_size() == 40
    assert [n for n, _ in solo_amd.solo_agc_params_t._fields_] == ["target_level", "max_boost_db", "max_cut_db", "sa_on_q8", "gate_level", "alpha_q8",
                                                                   "slew_up_q8", "slew_down_q8", "ceiling", "release_q15"]
    assert solo_amd.AGC_STATE_BYTES == host.emu_agc_state_bytes() == L.STATE_BYTES == 64
    hdr = open(os.path.join(T.ROOT, "include", "solo_mi355x.h")).read()
    assert "#define SOLO_AGC_STATE_BYTES 64" in hdr
    assert hasattr(solo_amd, "Agc") and solo_amd.Agc.COUNT == ("rows", "speech", "limited", "zero")
    st = np.full((3, 16), 0x5A5A5A5A, dtype=np.int32)
    host.emu_agc_init(st.ctypes.data, 3)
    assert np.array_equal(st, np.tile(np.array(M.INIT, dtype=np.int32), (3, 1))) and list(M.INIT[:5]) == [0, 0, 0, 65536, 32768]
    import inspect
    sig = inspect.signature(solo_amd.Agc.run)
    assert {k: v.default for k, v in sig.parameters.items() if k in M.DEFAULTS} == M.DEFAULTS


def test_solo_agc_refusals(host):
    buf = np.zeros(64, dtype=np.int16)
    a = (buf.ctypes.data + 15) & ~15                        # (never dereferenced: the checks look at addresses only)
    sa, cnt, rows = a + (1 << 20), a + (1 << 21), a + (1 << 22)
    far = a + (1 << 24)
    prm = lambda **kw: M.params_words(**kw)

    def ok(n_rows=8, rows=None, n=8, pcm=a, P=1, Ls=640, sa=None, frames=0, p=prm(), out=far, count=None):
        return host.emu_agc_call_ok(n_rows, rows, n, pcm, P, Ls, sa, frames, None if p is None else p.ctypes.data, out, count)
    assert ok() == 1 and ok(rows=rows, count=cnt, n=3) == 1 and ok(count=cnt) == 1 and ok(sa=sa, frames=2) == 1
    assert ok(pcm=None) == 0 and ok(out=None) == 0 and ok(p=None) == 0
    assert ok(rows=rows) == 0                               # d_count is required with d_rows
    for n in (0, -1, 9):
        assert ok(n=n) == 0
    assert ok(P=0) == 0 and ok(P=-1) == 0
    for Ls in (256, 288, 320, 640, 1280, 1888, 1920):
        assert ok(Ls=Ls) == 1, Ls
    for Ls in (0, -320, 32, 224, 255, 257, 300, 330, 648, 1921, 1952, 3200):
        assert ok(Ls=Ls) == 0, Ls
    assert ok(sa=sa, frames=0) == 0 and ok(sa=sa, frames=-1) == 0 and ok(frames=-1) == 1       # frames is ignored without d_sa_q8
    for off in (2, 4, 8):
        assert ok(pcm=a + off) == 0 and ok(out=far + off) == 0
    big = dict(n_rows=1 << 20, n=1 << 20, out=a)           # (in place: ranges of gigabytes)
    assert ok(P=4, Ls=640, **big) == 0                      # 2^31 samples and more
    assert ok(P=3, Ls=640, **big) == 1
    assert ok(P=2, Ls=256, sa=sa, frames=1024, **big) == 0 and ok(P=2, Ls=256, sa=sa, frames=1023, **big) == 1
    assert ok(P=2, Ls=256, frames=1 << 20, **big) == 1
    # in place, apart, partial overlap (8 rows x 640 samples = 10240 bytes)
    assert ok(out=a) == 1 and ok(out=a + 10240) == 1 and ok(pcm=a + 10240, out=a) == 1
    for d in (16, 640, 10224):
        assert ok(out=a + d) == 0 and ok(pcm=a + d, out=a) == 0, d
    lo = dict(target=0, boost=0, cut=0, sa_on=0, gate=0, alpha=1, up=0, down=0, ceiling=1, release=0)
    hi = dict(target=127, boost=30, cut=30, sa_on=255, gate=127, alpha=256, up=7680, down=7680, ceiling=32767, release=32768)
    assert ok(p=prm(**lo)) == 1 and ok(p=prm(**hi)) == 1
    for k in M.PARAMS:
        assert ok(p=prm(**{k: lo[k] - 1})) == 0 and ok(p=prm(**{k: hi[k] + 1})) == 0, k
        assert ok(p=prm(**{k: lo[k]})) == 1 and ok(p=prm(**{k: hi[k]})) == 1, k
    kept = []

    def arr(v):
        kept.append(np.array(v, dtype=np.int32))
        return kept[-1].ctypes.data
    assert host.emu_agc_list_ok(arr([0, 2]), 2, 4) == 1 and host.emu_agc_list_ok(arr([2, 0]), 2, 4) == 1
    assert host.emu_agc_list_ok(arr([0, 0]), 2, 4) == 0 and host.emu_agc_list_ok(arr([0, 4]), 2, 4) == 0 and host.emu_agc_list_ok(arr([-1]), 1, 4) == 0
    assert host.emu_agc_list_ok(arr([0, 1, 2, 3, 0]), 5, 4) == 0 and host.emu_agc_list_ok(None, 1, 4) == 0 and host.emu_agc_list_ok(arr([0]), 0, 4) == 0
    # the run entry of the host build makes the same checks
    e = L.HostEngine(host, 2)
    x = L.rows_pcm(1, 2, 1, 320)
    assert e.run(x, None, None, None, False, ceiling=0) is None and e.status == -1 and np.array_equal(e.state(), M.Agc(2).state_bytes())

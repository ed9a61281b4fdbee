"""Read side of the receiver ring (solo_recv_track, solo_recv_report): declared in the header, exported by the built library, bound by
solo_amd with their argument types; both structures have the same size and field order in the header, in ctypes and in
SoloBatch.RECV_REPORT; a NULL handle is refused whatever else is passed; the Python checks of recv_report() raise before anything
reaches the library.  No compute call (no GPU here; the refusals that need a handle are in tests/test_gpu_recv_report.py)."""
import ctypes as C
import re

import pytest

import solo_amd
import solo_testlib as T
from recv_report_model import FIELDS

NEW = {"solo_recv_track": 3, "solo_recv_report": 12}


@pytest.fixture(scope="module")
def lib():
    return T.built_library()


def test_declared_exported_bound(lib):
    hdr = T.header_text()
    loaded = solo_amd.load_library()
    for n, nargs in NEW.items():
        m = re.search(r"\bint32_t\s+%s\s*\(([^)]*)\)" % n, hdr)
        assert m, n
        assert len(m.group(1).split(",")) == nargs, n
        assert hasattr(lib, n), n
        assert n in solo_amd.ABI_SYMBOLS, n
        f = getattr(loaded, n)
        assert f.restype is C.c_int32 and len(f.argtypes) == nargs, n
    args = [a.strip() for a in re.search(r"solo_recv_report\s*\(([^)]*)\)", hdr).group(1).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["b", "d_streams", "n", "d_min_ready", "min_ready", "max_span", "flags", "d_reports", "d_play_list",
                                                         "d_play_rows", "d_count", "hip_stream"]
    assert [loaded.solo_recv_report.argtypes[i] for i in (2, 4, 5, 6)] == [C.c_int32] * 4
    assert re.search(r"#define\s+SOLO_RECV_REPORT_CLEAR_MARGIN\s+1\b", hdr) and solo_amd.RECV_REPORT_CLEAR_MARGIN == 1


def _struct_fields(name):
    m = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % name, T.header_text())
    assert m, name
    fields = re.findall(r"(int32_t|uint32_t)\s+([^;]+);", m.group(1))
    return [(ty, x.strip()) for ty, group in fields for x in group.split(",")]


def test_structs_agree_on_all_sides():
    rep = _struct_fields("solo_recv_report_t")
    assert 4 * len(rep) == 64 == C.sizeof(solo_amd.solo_recv_report_t)
    assert [n for _, n in rep] == [f[0] for f in solo_amd.solo_recv_report_t._fields_] == list(solo_amd.SoloBatch.RECV_REPORT) == list(FIELDS)
    for (ty, n), (_, ct) in zip(rep, solo_amd.solo_recv_report_t._fields_):
        assert ct is (C.c_int32 if ty == "int32_t" else C.c_uint32), n
    assert [getattr(solo_amd.solo_recv_report_t, n).offset for n in FIELDS] == list(range(0, 64, 4))
    cnt = _struct_fields("solo_recv_report_count_t")
    assert [n for _, n in cnt] == ["selected", "listed"] == [f[0] for f in solo_amd.solo_recv_report_count_t._fields_]
    assert 4 * len(cnt) == 8 == C.sizeof(solo_amd.solo_recv_report_count_t)


def test_null_handle_is_refused(lib):
    loaded = solo_amd.load_library()
    x = (C.c_int32 * 64)()
    p = C.cast(x, C.c_void_p)
    assert loaded.solo_recv_track(None, 1, None) == -1 and loaded.solo_recv_track(None, 0, None) == -1
    assert loaded.solo_recv_report(None, None, 1, None, 0, 0, 0, p, p, p, p, None) == -1
    assert loaded.solo_recv_report(None, p, 1, p, 1, 1, 1, p, None, None, None, None) == -1


def _batch(n_streams=8):
    torch = pytest.importorskip("torch")
    b = object.__new__(solo_amd.SoloBatch)
    b.torch, b.lib, b.h = torch, T.NoLib(), None
    b.n_streams, b.slot, b.packet_samples, b.device = n_streams, 512, 640, torch.device("cpu")
    return b, torch


def test_python_checks_raise_before_the_library():
    b, t = _batch()
    bad = [
        dict(streams=[3, 1]), dict(streams=[2, 2]), dict(streams=[0, 8]), dict(streams=[]), dict(streams=list(range(9))),
        dict(streams=T.FakeDev((3,), t.int64)), dict(streams=T.FakeDev((3, 1), t.int32)), dict(streams=T.FakeDev((9,), t.int32)),
        dict(streams=T.FakeDev((0,), t.int32)), dict(streams=T.FakeDev((3,), t.int32, contiguous=False)),
        dict(min_ready=1.5), dict(min_ready=True), dict(min_ready=T.FakeDev((7,), t.int32)), dict(min_ready=T.FakeDev((8,), t.int16)),
        dict(min_ready=T.FakeDev((8,), t.int32, cuda=False)), dict(min_ready=2 ** 31), dict(max_span=2 ** 31),
        dict(streams=T.FakeDev((3,), t.int32), min_ready=T.FakeDev((8,), t.int32)),
        dict(reports=T.FakeDev((8, 15), t.int32)), dict(reports=T.FakeDev((8, 16), t.uint8)), dict(reports=T.FakeDev((7, 16), t.int32)),
        dict(play_list=T.FakeDev((7,), t.int32)), dict(play_list=T.FakeDev((8,), t.int64)), dict(play_rows=T.FakeDev((8, 1), t.int32)),
        dict(play_rows=T.FakeDev((8,), t.int32, cuda=False)),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            b.recv_report(**kw)


def test_signature():
    import inspect
    assert list(inspect.signature(solo_amd.SoloBatch.recv_report).parameters) == ["self", "streams", "min_ready", "max_span", "clear_margin", "reports",
                                                                                  "play_list", "play_rows"]
    assert list(inspect.signature(solo_amd.SoloBatch.recv_track).parameters) == ["self", "on"]
    assert list(inspect.signature(solo_amd.SoloBatch.recv_report_count).parameters) == ["self", "count"]

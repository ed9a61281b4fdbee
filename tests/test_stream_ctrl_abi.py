"""Per-stream control and stream lifecycle in a batch handle (solo_batch_reset_streams, solo_recv_reset_streams): declared in the
header, exported by the built library, bound by solo_amd.  No compute call (no GPU here)."""
import ctypes as C
import os
import re

import pytest

import solo_amd
import solo_testlib as T

NEW = ("solo_batch_reset_streams", "solo_recv_reset_streams")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(solo_amd.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return C.CDLL(solo_amd.LIB_PATH)


def test_declared_exported_and_listed(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(T.ROOT, "include", "solo_mi355x.h")).read(), flags=re.S)
    for n in NEW:
        assert re.search(r"\bint32_t\s+%s\s*\(" % n, hdr), n
        assert hasattr(lib, n), n
        assert n in solo_amd.ABI_SYMBOLS, n


def test_binding_has_the_methods():
    assert callable(getattr(solo_amd.SoloBatch, "reset_streams", None))
    assert callable(getattr(solo_amd.SoloBatch, "recv_reset_streams", None))
    loaded = solo_amd.load_library()
    assert loaded.solo_batch_reset_streams.restype is C.c_int32 and len(loaded.solo_batch_reset_streams.argtypes) == 7
    assert loaded.solo_recv_reset_streams.restype is C.c_int32 and len(loaded.solo_recv_reset_streams.argtypes) == 5


def test_null_handle_is_refused(lib):
    idx = (C.c_int32 * 1)(0)
    lib.solo_batch_reset_streams.restype = C.c_int32
    lib.solo_recv_reset_streams.restype = C.c_int32
    assert lib.solo_batch_reset_streams(None, idx, 1, 3, None, None, None) == -1
    assert lib.solo_recv_reset_streams(None, idx, 1, idx, None) == -1

"""Sender back end (solo_send_pack, solo_send_pack_streams): declared in the header, exported by the built library, bound by solo_amd
with their argument types; the count structure is 32 bytes on both sides; a NULL handle and bad counts are refused; the Python checks of
send_pack() raise before anything reaches the library.  No compute call (no GPU here)."""
import ctypes as C
import re

import pytest

import solo_amd
import solo_testlib as T

NEW = {"solo_send_pack": 13, "solo_send_pack_streams": 15}


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
        assert f.argtypes[-3] is C.c_int64, n                      # payload_capacity
    assert "const int32_t *d_streams" in re.search(r"solo_send_pack_streams\s*\(([^)]*)\)", hdr).group(1)
    assert loaded.solo_send_pack_streams.argtypes[2] is C.c_int32


def test_count_struct_is_32_bytes_on_both_sides():
    m = re.search(r"typedef struct \{([^}]*)\}\s*solo_send_count_t;", T.header_text())
    assert m
    fields = re.findall(r"(int32_t|int64_t)\s+([^;]+);", m.group(1))
    names = [x.strip() for _, group in fields for x in group.split(",")]
    size = sum((4 if ty == "int32_t" else 8) * len(group.split(",")) for ty, group in fields)
    assert size == 32 == C.sizeof(solo_amd.solo_send_count_t)
    assert names == [f[0] for f in solo_amd.solo_send_count_t._fields_] == list(solo_amd.SoloBatch.SEND_COUNT)
    assert solo_amd.solo_send_count_t.bytes.offset == 8 and solo_amd.solo_send_count_t.empty.offset == 24


def test_null_handle_and_bad_counts_are_refused(lib):
    loaded = solo_amd.load_library()
    x = (C.c_int32 * 16)()
    p = C.cast(x, C.c_void_p)
    assert loaded.solo_send_pack(None, p, p, None, 1, None, 0, p, 1, p, 1, p, None) == -1
    assert loaded.solo_send_pack_streams(None, p, 1, p, p, None, 1, None, 0, p, 1, p, 1, p, None) == -1


def _batch(n_streams=8):
    torch = pytest.importorskip("torch")
    b = object.__new__(solo_amd.SoloBatch)
    b.torch, b.lib, b.h = torch, T.NoLib(), None
    b.n_streams, b.slot, b.packet_samples, b.device = n_streams, 512, 640, torch.device("cpu")
    return b, torch


def test_python_checks_raise_before_the_library():
    b, t = _batch()
    bits, nb = T.FakeDev((8, 3, 512), t.uint8), T.FakeDev((8, 3, 2), t.int16)
    bad = [
        dict(bits=T.FakeDev((8, 3, 256), t.uint8), nbytes=nb),                           # another slot size
        dict(bits=T.FakeDev((7, 3, 512), t.uint8), nbytes=T.FakeDev((7, 3, 2), t.int16)),  # rows != N without a list
        dict(bits=T.FakeDev((8, 3, 512), t.int8), nbytes=nb),
        dict(bits=T.FakeDev((8, 3, 512), t.uint8, cuda=False), nbytes=nb),
        dict(bits=T.FakeDev((8, 3, 512), t.uint8, contiguous=False), nbytes=nb),
        dict(bits=T.FakeDev((8, 0, 512), t.uint8), nbytes=T.FakeDev((8, 0, 2), t.int16)),
        dict(bits=bits, nbytes=T.FakeDev((8, 3), t.int16)),
        dict(bits=bits, nbytes=T.FakeDev((8, 3, 2), t.int32)),
        dict(bits=bits, nbytes=nb, send=T.FakeDev((8, 4), t.uint8)),
        dict(bits=bits, nbytes=nb, send=T.FakeDev((8, 3), t.int32)),
        dict(bits=bits, nbytes=nb, seq_base=T.FakeDev((7,), t.int32)),
        dict(bits=bits, nbytes=nb, seq_base=T.FakeDev((8,), t.int64)),
        dict(bits=bits, nbytes=nb, first_seq=2 ** 31),
        dict(bits=bits, nbytes=nb, records=T.FakeDev((10, 4), t.int32)),
        dict(bits=bits, nbytes=nb, records=T.FakeDev((10, 5), t.int64)),
        dict(bits=bits, nbytes=nb, payload=T.FakeDev((10, 5), t.uint8)),
        dict(bits=bits, nbytes=nb, payload=T.FakeDev((10,), t.int8)),
        dict(bits=bits, nbytes=nb, streams=[0, 1, 2]),                                  # rows != listed streams
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            b.send_pack(**kw)


@pytest.mark.parametrize("streams", [[], [3, 1], [2, 2], [0, 8], [-1, 2], list(range(9))])
def test_stream_lists_are_checked_before_the_library(streams):
    b, t = _batch()
    n = max(len(streams), 1)
    with pytest.raises(ValueError):
        b.send_pack(T.FakeDev((n, 1, 512), t.uint8), T.FakeDev((n, 1, 2), t.int16), streams=streams)


def test_signature():
    import inspect
    assert list(inspect.signature(solo_amd.SoloBatch.send_pack).parameters) == ["self", "bits", "nbytes", "send", "first_seq", "seq_base", "records",
                                                                                "payload", "streams"]

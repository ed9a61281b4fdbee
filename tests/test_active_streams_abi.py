"""Subset calls of a batch handle (solo_batch_encode_streams, solo_batch_decode_streams, solo_recv_decode_streams): declared in the
header, exported by the built library, bound by solo_amd with their argument types; the Python checks of `streams=` raise before
anything reaches the library; the mapped quantiser instances keep the quantiser's budgets.  No compute call (no GPU here)."""
import ctypes as C
import os
import re
import sys

import pytest

import solo_amd
import solo_testlib as T

NEW = {"solo_batch_encode_streams": 9, "solo_batch_decode_streams": 10, "solo_recv_decode_streams": 7}


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
        assert "const int32_t *d_streams" in m.group(1), n
        assert hasattr(lib, n), n
        assert n in solo_amd.ABI_SYMBOLS, n
        f = getattr(loaded, n)
        assert f.restype is C.c_int32 and len(f.argtypes) == nargs, n
        assert f.argtypes[2] is C.c_int32, n                      # the count follows the handle and the list


def test_null_handle_and_bad_counts_are_refused(lib):
    for n in NEW:
        getattr(lib, n).restype = C.c_int32
    idx = (C.c_int32 * 1)(0)
    assert lib.solo_batch_encode_streams(None, idx, 1, idx, 1, idx, idx, None, None) == -1
    assert lib.solo_batch_decode_streams(None, idx, 1, idx, idx, None, 1, idx, None, None) == -1
    assert lib.solo_recv_decode_streams(None, idx, 1, 1, idx, None, None) == -1


def _batch(n_streams=8):
    torch = pytest.importorskip("torch")
    b = object.__new__(solo_amd.SoloBatch)
    b.torch, b.lib, b.h = torch, T.NoLib(), None
    b.n_streams, b.slot, b.packet_samples, b.device = n_streams, 512, 640, torch.device("cpu")
    return b, torch


@pytest.mark.parametrize("streams", [[], [3, 1], [2, 2], [0, 8], [-1, 2], list(range(9))])
def test_python_checks_raise_before_the_library(streams):
    b, torch = _batch()
    n = max(len(streams), 1)
    with pytest.raises(ValueError):
        b.encode(T.FakeDev((n, 1, 640), torch.int16), streams=streams)
    with pytest.raises(ValueError):
        b.decode(T.FakeDev((n, 1, 512), torch.uint8), T.FakeDev((n, 1, 2), torch.int16), streams=streams)
    with pytest.raises(ValueError):
        b.recv_decode(1, streams=streams)


def test_rows_must_match_the_list():
    b, torch = _batch()
    with pytest.raises(ValueError):
        b.encode(T.FakeDev((3, 1, 640), torch.int16), streams=[0, 1])
    with pytest.raises(ValueError):
        b.decode(T.FakeDev((8, 1, 512), torch.uint8), T.FakeDev((8, 1, 2), torch.int16), streams=[0, 5])


def test_positional_signatures_unchanged():
    import inspect
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(solo_amd.SoloBatch.encode)[:5] == ["self", "pcm", "bits", "nbytes", "status"]
    assert sig(solo_amd.SoloBatch.decode)[:6] == ["self", "bits", "nbytes", "recv", "pcm", "status"]
    assert sig(solo_amd.SoloBatch.recv_decode)[:4] == ["self", "n_packets", "pcm", "status"]
    for f in (solo_amd.SoloBatch.encode, solo_amd.SoloBatch.decode, solo_amd.SoloBatch.recv_decode):
        assert inspect.signature(f).parameters["streams"].default is None


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="no LLVM binutils on this box")
def test_mapped_quantiser_within_the_quantiser_budget(lib):
    """The mapped quantiser instances (subset calls) keep the register allocation of the identity instance and use no scratch
    beyond it: a register more would take a wave per SIMD away from the residency plan."""
    sys.path.insert(0, os.path.join(T.ROOT, "tools"))
    from kernel_resources import kernel_resources
    seen = kernel_resources(solo_amd.LIB_PATH)
    for suffix in ("", "_wb"):
        ident, mapped = seen["solo_nsq_kernel" + suffix], seen["solo_nsq_kernel_mapped" + suffix]
        assert mapped["vgpr_alloc"] <= ident["vgpr_alloc"], (suffix, mapped, ident)
        assert mapped["scratch"] <= ident["scratch"] and mapped["lds"] <= ident["lds"], (suffix, mapped, ident)
    assert seen["solo_nsq_kernel_mapped"]["vgpr_alloc"] <= 128

"""Play-out time scaling (solo_timescale): declared in the header, exported by the built library, bound by solo_amd with its argument types;
the count structure is 16 bytes on both sides with `cost` at offset 8; a NULL handle is refused; the Python checks of timescale() raise
before anything reaches the library; the new kernels of the built library use no scratch.  No compute call (no GPU here)."""
import ctypes as C
import inspect
import os
import re
import sys

import pytest

import solo_amd
import solo_testlib as T

KERNELS = ("solo_timescale_count_kernel", "solo_timescale_kernel")


@pytest.fixture(scope="module")
def lib():
    return T.built_library()


def test_declared_exported_bound(lib):
    m = re.search(r"\bint32_t\s+solo_timescale\s*\(([^)]*)\)", T.header_text())
    assert m
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["solo_batch_t *b", "const int16_t *d_pcm_in", "int32_t n", "int32_t in_packets", "int32_t out_packets", "int16_t *d_pcm_out",
                    "int32_t *d_shift", "int32_t *d_cost", "solo_timescale_count_t *d_count", "void *hip_stream"]
    assert hasattr(lib, "solo_timescale") and "solo_timescale" in solo_amd.ABI_SYMBOLS
    f = solo_amd.load_library().solo_timescale
    assert f.restype is C.c_int32 and len(f.argtypes) == 10
    assert [i for i, t in enumerate(f.argtypes) if t is C.c_int32] == [2, 3, 4]             # n, in_packets, out_packets
    assert all(t is C.c_void_p for i, t in enumerate(f.argtypes) if i not in (2, 3, 4))


def test_count_struct_is_16_bytes_on_both_sides():
    m = re.search(r"typedef struct \{([^}]*)\}\s*solo_timescale_count_t;", T.header_text())
    assert m
    fields = re.findall(r"(int32_t|int64_t)\s+([^;]+);", m.group(1))
    names = [x.strip() for _, group in fields for x in group.split(",")]
    size = sum((4 if ty == "int32_t" else 8) * len(group.split(",")) for ty, group in fields)
    assert size == 16 == C.sizeof(solo_amd.solo_timescale_count_t)
    assert names == [f[0] for f in solo_amd.solo_timescale_count_t._fields_] == list(solo_amd.SoloBatch.TIMESCALE_COUNT) == ["rows", "blocks", "cost"]
    assert solo_amd.solo_timescale_count_t.cost.offset == 8 and solo_amd.solo_timescale_count_t.cost.size == 8


def test_null_handle_is_refused(lib):
    x = (C.c_int32 * 2048)()
    base = C.addressof(x)
    p_in = C.c_void_p((base + 15) & ~15)
    p_out = C.c_void_p(((base + 15) & ~15) + 4096)
    assert solo_amd.load_library().solo_timescale(None, p_in, 1, 2, 1, p_out, None, None, None, None) == -1


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="no LLVM binutils on this box")
def test_timescale_kernels_use_no_scratch(lib):
    sys.path.insert(0, os.path.join(T.ROOT, "tools"))
    from kernel_resources import kernel_resources
    seen = kernel_resources(solo_amd.LIB_PATH)
    for frag in KERNELS:
        hits = [r for name, r in seen.items() if re.search(r"\d%s(?![a-z_])" % frag, name)]
        assert len(hits) == 1, (frag, len(hits))                  # rate-independent: compiled once
        assert hits[0]["scratch"] == 0, (frag, hits[0])


def test_python_checks_raise_before_the_library():
    t = pytest.importorskip("torch")
    b = object.__new__(solo_amd.SoloBatch)
    b.torch, b.lib, b.h = t, T.NoLib(), None
    b.n_streams, b.slot, b.packet_samples, b.samplerate, b.device = 8, 512, 640, 16000, t.device("cpu")
    pcm = T.FakeDev((8, 2, 640), t.int16)
    bad = [
        dict(pcm=T.FakeDev((8, 2, 1280), t.int16), out_packets=1),                   # another packet length
        dict(pcm=T.FakeDev((8, 2, 640), t.int32), out_packets=1),
        dict(pcm=T.FakeDev((8, 2, 640), t.int16, cuda=False), out_packets=1),
        dict(pcm=T.FakeDev((8, 2, 640), t.int16, contiguous=False), out_packets=1),
        dict(pcm=T.FakeDev((8, 640), t.int16), out_packets=1),
        dict(pcm=T.FakeDev((0, 2, 640), t.int16), out_packets=1),
        dict(pcm=T.FakeDev((8, 0, 640), t.int16), out_packets=1),
        dict(pcm=T.FakeDev((8, 5, 640), t.int16), out_packets=1),
        dict(pcm=pcm, out_packets=0),
        dict(pcm=pcm, out_packets=5),
        dict(pcm=T.FakeDev((2 ** 20, 2, 640), t.int16), out_packets=4),              # n x max(a, b) x L = 2^31
        dict(pcm=pcm, out_packets=1, out=T.FakeDev((8, 2, 640), t.int16)),
        dict(pcm=pcm, out_packets=1, out=T.FakeDev((8, 1, 640), t.int32)),
        dict(pcm=pcm, out_packets=1, out=T.FakeDev((8, 1, 640), t.int16, contiguous=False)),
        dict(pcm=pcm, out_packets=1, shift=T.FakeDev((8, 7), t.int32)),              # M = 640 / 80 = 8 blocks
        dict(pcm=pcm, out_packets=1, shift=T.FakeDev((8, 8), t.int64)),
        dict(pcm=pcm, out_packets=3, cost=T.FakeDev((8, 8), t.int32)),               # M = 24
        dict(pcm=pcm, out_packets=1, cost=T.FakeDev((8, 8), t.int32, cuda=False)),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            b.timescale(**kw)


def test_signature():
    assert list(inspect.signature(solo_amd.SoloBatch.timescale).parameters) == ["self", "pcm", "out_packets", "out", "shift", "cost"]
    assert list(inspect.signature(solo_amd.SoloBatch.timescale_count).parameters) == ["self", "count"]

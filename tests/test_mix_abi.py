"""Mixing bridge (solo_mix): declared in the header, exported by the built library, bound by solo_amd with its argument types; the count
structure is 16 bytes on both sides; a NULL handle is refused; the Python checks of mix() raise before anything reaches the library; the
new kernels of the built library use no scratch.  No compute call (no GPU here)."""
import ctypes as C
import inspect
import os
import re
import sys

import pytest

import solo_amd
import solo_testlib as T

KERNELS = ("solo_mix_clear_kernel", "solo_mix_check_kernel", "solo_mix_scan_kernel", "solo_mix_scatter_kernel", "solo_mix_kernel")


@pytest.fixture(scope="module")
def lib():
    return T.built_library()


def test_declared_exported_bound(lib):
    m = re.search(r"\bint32_t\s+solo_mix\s*\(([^)]*)\)", T.header_text())
    assert m
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 13
    assert args[1] == "const int16_t *d_pcm_in" and args[4] == "const int32_t *d_room" and args[8] == "int16_t *d_pcm_out"
    assert args[9] == "int64_t *d_energy" and args[10] == "uint8_t *d_mixed" and args[11] == "solo_mix_count_t *d_count"
    assert hasattr(lib, "solo_mix") and "solo_mix" in solo_amd.ABI_SYMBOLS
    f = solo_amd.load_library().solo_mix
    assert f.restype is C.c_int32 and len(f.argtypes) == 13
    assert [i for i, t in enumerate(f.argtypes) if t is C.c_int32] == [2, 3, 5, 7]          # n, n_packets, n_rooms, max_speakers


def test_count_struct_is_16_bytes_on_both_sides():
    m = re.search(r"typedef struct \{([^}]*)\}\s*solo_mix_count_t;", T.header_text())
    assert m
    fields = re.findall(r"(int32_t|int64_t)\s+([^;]+);", m.group(1))
    names = [x.strip() for _, group in fields for x in group.split(",")]
    size = sum((4 if ty == "int32_t" else 8) * len(group.split(",")) for ty, group in fields)
    assert size == 16 == C.sizeof(solo_amd.solo_mix_count_t)
    assert names == [f[0] for f in solo_amd.solo_mix_count_t._fields_] == list(solo_amd.SoloBatch.MIX_COUNT)
    assert solo_amd.solo_mix_count_t.clipped.offset == 8


def test_null_handle_is_refused(lib):
    x = (C.c_int32 * 64)()
    p = C.cast(x, C.c_void_p)
    assert solo_amd.load_library().solo_mix(None, p, 1, 1, p, 1, None, 0, p, None, None, None, None) == -1


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="no LLVM binutils on this box")
def test_mix_kernels_use_no_scratch(lib):
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
    b.n_streams, b.slot, b.packet_samples, b.device = 8, 512, 640, t.device("cpu")
    pcm, room = T.FakeDev((8, 3, 640), t.int16), T.FakeDev((8,), t.int32)
    bad = [
        dict(pcm=T.FakeDev((8, 3, 1280), t.int16), room=room),                       # another packet length
        dict(pcm=T.FakeDev((8, 3, 640), t.int32), room=room),
        dict(pcm=T.FakeDev((8, 3, 640), t.int16, cuda=False), room=room),
        dict(pcm=T.FakeDev((8, 3, 640), t.int16, contiguous=False), room=room),
        dict(pcm=T.FakeDev((8, 0, 640), t.int16), room=room),
        dict(pcm=T.FakeDev((8, 640), t.int16), room=room),
        dict(pcm=pcm, room=T.FakeDev((7,), t.int32)),
        dict(pcm=pcm, room=T.FakeDev((8,), t.int64)),
        dict(pcm=pcm, room=room, gain=T.FakeDev((8,), t.int32)),
        dict(pcm=pcm, room=room, gain=T.FakeDev((9,), t.int16)),
        dict(pcm=pcm, room=room, max_speakers=65),
        dict(pcm=T.FakeDev((8192, 1, 640), t.int16), room=T.FakeDev((8192,), t.int32), max_speakers=0),
        dict(pcm=pcm, room=room, out=T.FakeDev((8, 3, 320), t.int16)),
        dict(pcm=pcm, room=room, out=T.FakeDev((8, 3, 640), t.int32)),
        dict(pcm=pcm, room=room, energy=T.FakeDev((8, 3), t.int32)),
        dict(pcm=pcm, room=room, energy=T.FakeDev((8, 4), t.int64)),
        dict(pcm=pcm, room=room, mixed=T.FakeDev((8, 3), t.int8)),
        dict(pcm=pcm, room=room, mixed=T.FakeDev((3, 8), t.uint8)),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            b.mix(**kw)


def test_signature():
    assert list(inspect.signature(solo_amd.SoloBatch.mix).parameters) == ["self", "pcm", "room", "gain", "max_speakers", "out", "energy", "mixed"]
    assert list(inspect.signature(solo_amd.SoloBatch.mix_count).parameters) == ["self", "count"]

"""Shared listener mixes from a given selection (solo_mix_selected): declared in the header, exported by the built library, bound by
solo_amd with its 20 argument types and listed in ABI_SYMBOLS; the count structure is 32 bytes on both sides; a NULL handle is refused;
the Python checks raise before anything reaches the library; the new kernels exist once each and use no scratch, and the gather and
write passes no LDS.  No compute call (no GPU here)."""
import ctypes as C
import inspect
import os
import re
import sys

import pytest

import solo_amd
import solo_testlib as T

KERNELS = ("solo_mixsel_gather_kernel", "solo_mixsel_compact_kernel", "solo_mixsel_write_kernel")


@pytest.fixture(scope="module")
def lib():
    return T.built_library()


def test_mix_selected_declared_exported_bound(lib):
    m = re.search(r"\bint32_t\s+solo_mix_selected\s*\(([^)]*)\)", T.header_text())
    assert m
    args = [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]
    assert args == ["solo_batch_t *b", "const int16_t *d_pcm_in", "int32_t n", "int32_t n_packets", "const int32_t *d_room", "int32_t n_rooms",
                    "const int16_t *d_gain_q12", "const uint8_t *d_sel", "const uint8_t *d_keep", "const int32_t *d_slots", "int16_t *d_pcm_spk",
                    "int32_t *d_spk_list", "int32_t *d_spk_rows", "int16_t *d_pcm_room", "int32_t *d_room_list", "int32_t *d_source",
                    "uint8_t *d_room_nsel", "int64_t *d_energy", "solo_mix_selected_count_t *d_count", "void *hip_stream"]
    assert hasattr(lib, "solo_mix_selected") and "solo_mix_selected" in solo_amd.ABI_SYMBOLS
    f = solo_amd.load_library().solo_mix_selected
    assert f.restype is C.c_int32 and len(f.argtypes) == 20
    assert [i for i, t in enumerate(f.argtypes) if t is C.c_int32] == [2, 3, 5]              # n, n_packets, n_rooms
    assert all(t is C.c_void_p for i, t in enumerate(f.argtypes) if i not in (2, 3, 5))


def test_count_struct_is_32_bytes_on_both_sides():
    m = re.search(r"typedef struct \{([^}]*)\}\s*solo_mix_selected_count_t;", T.header_text())
    assert m
    fields = re.findall(r"(int32_t|int64_t)\s+([^;]+);", m.group(1))
    names = [x.strip() for _, group in fields for x in group.split(",")]
    size = sum((4 if ty == "int32_t" else 8) * len(group.split(",")) for ty, group in fields)
    assert size == 32 == C.sizeof(solo_amd.solo_mix_selected_count_t)
    assert names == [f[0] for f in solo_amd.solo_mix_selected_count_t._fields_] == list(solo_amd.SoloBatch.MIX_SELECTED_COUNT)
    assert solo_amd.solo_mix_selected_count_t.clipped.offset == 16 and solo_amd.solo_mix_selected_count_t.selected.offset == 24
    # the first 24 bytes are solo_mix_shared_count_t
    assert solo_amd.solo_mix_selected_count_t._fields_[:5] == solo_amd.solo_mix_shared_count_t._fields_


def test_null_handle_is_refused(lib):
    x = (C.c_int32 * 64)()
    p = C.cast(x, C.c_void_p)
    assert solo_amd.load_library().solo_mix_selected(None, p, 1, 1, p, 1, None, p, None, None, p, p, p, p, p, p, None, None, p, None) == -1


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="no LLVM binutils on this box")
def test_kernels_exist_once_and_use_no_scratch(lib):
    sys.path.insert(0, os.path.join(T.ROOT, "tools"))
    from kernel_resources import kernel_resources
    seen = kernel_resources(solo_amd.LIB_PATH)
    for frag in KERNELS:
        hits = [r for name, r in seen.items() if re.search(r"\d%s(?![a-z_])" % frag, name)]
        assert len(hits) == 1, (frag, len(hits))                  # rate-independent: compiled once
        assert hits[0]["scratch"] == 0, (frag, hits[0])
        if frag != "solo_mixsel_compact_kernel":
            assert hits[0]["lds"] == 0, (frag, hits[0])           # nothing but registers bounds the waves per SIMD
    assert len([name for name in seen if "solo_mixsel_" in name]) == len(KERNELS)


def test_python_checks_of_mix_selected_raise_before_the_library():
    t = pytest.importorskip("torch")
    b = object.__new__(solo_amd.SoloBatch)
    b.torch, b.lib, b.h = t, T.NoLib(), None
    b.n_streams, b.slot, b.packet_samples, b.device = 8, 512, 640, t.device("cpu")
    pcm, room, sel = T.FakeDev((8, 3, 640), t.int16), T.FakeDev((8,), t.int32), T.FakeDev((8, 3), t.uint8)
    bad = [
        dict(pcm=T.FakeDev((8, 3, 1280), t.int16), room=room, sel=sel),
        dict(pcm=T.FakeDev((8, 3, 640), t.int16, cuda=False), room=room, sel=sel),
        dict(pcm=T.FakeDev((8, 3, 640), t.int16, contiguous=False), room=room, sel=sel),
        dict(pcm=T.FakeDev((8, 0, 640), t.int16), room=room, sel=T.FakeDev((8, 0), t.uint8)),
        dict(pcm=pcm, room=T.FakeDev((7,), t.int32), sel=sel),
        dict(pcm=pcm, room=T.FakeDev((8,), t.int64), sel=sel),
        dict(pcm=pcm, room=room, sel=None),
        dict(pcm=pcm, room=room, sel=T.FakeDev((8, 3), t.int8)),
        dict(pcm=pcm, room=room, sel=T.FakeDev((8, 3), t.bool)),
        dict(pcm=pcm, room=room, sel=T.FakeDev((8,), t.uint8)),
        dict(pcm=pcm, room=room, sel=T.FakeDev((8, 2), t.uint8)),
        dict(pcm=pcm, room=room, sel=T.FakeDev((8, 3), t.uint8, cuda=False)),
        dict(pcm=pcm, room=room, sel=T.FakeDev((8, 3), t.uint8, contiguous=False)),
        dict(pcm=pcm, room=room, sel=sel, gain=T.FakeDev((9,), t.int16)),
        dict(pcm=pcm, room=room, sel=sel, keep=T.FakeDev((8,), t.int8)),
        dict(pcm=pcm, room=room, sel=sel, keep=T.FakeDev((8, 3), t.uint8)),
        dict(pcm=pcm, room=room, sel=sel, slots=T.FakeDev((8,), t.int64)),
        dict(pcm=pcm, room=room, sel=sel, slots=T.FakeDev((7,), t.int32)),
        dict(pcm=pcm, room=room, sel=sel, n_rooms=0),
        dict(pcm=pcm, room=room, sel=sel, n_rooms=9),
        dict(pcm=pcm, room=room, sel=sel, energy=T.FakeDev((8, 4), t.int64)),
        dict(pcm=pcm, room=room, sel=sel, energy=T.FakeDev((8, 3), t.int32)),
        dict(pcm=pcm, room=room, sel=sel, n_rooms=4, room_nsel=T.FakeDev((8, 3), t.uint8)),
        dict(pcm=pcm, room=room, sel=sel, room_nsel=T.FakeDev((8, 3), t.int8)),
        dict(pcm=pcm, room=room, sel=sel, pcm_spk=T.FakeDev((7, 3, 640), t.int16)),
        dict(pcm=pcm, room=room, sel=sel, n_rooms=4, pcm_room=T.FakeDev((8, 3, 640), t.int16)),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            b.mix_selected(**kw)


def test_signatures():
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(solo_amd.SoloBatch.mix_selected) == ["self", "pcm", "room", "sel", "gain", "keep", "slots", "n_rooms", "energy", "room_nsel", "pcm_spk",
                                                    "pcm_room"]
    assert all(p.default is None for name, p in inspect.signature(solo_amd.SoloBatch.mix_selected).parameters.items()
               if name not in ("self", "pcm", "room", "sel"))
    assert sig(solo_amd.SoloBatch.mix_selected_count) == ["self", "count"]
    assert solo_amd.SoloBatch.MIX_SELECTED_COUNT[:5] == solo_amd.SoloBatch.MIX_SHARED_COUNT

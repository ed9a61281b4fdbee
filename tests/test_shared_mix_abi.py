"""Shared listener mixes (solo_mix_shared, solo_send_fanout): declared in the header, exported by the built library, bound by solo_amd with
their argument types and listed in ABI_SYMBOLS; the count structure is 24 bytes on both sides; a NULL handle is refused; the Python checks
raise before anything reaches the library; the new kernels use no scratch, and the energy pass no LDS.  No compute call (no GPU here)."""
import ctypes as C
import inspect
import os
import re
import sys

import pytest

import solo_amd
import solo_testlib as T

KERNELS = ("solo_mixsh_clear_kernel", "solo_mixsh_check_kernel", "solo_mixsh_energy_kernel", "solo_mixsh_select_kernel", "solo_mixsh_tally_kernel",
           "solo_mixsh_compact_kernel", "solo_mixsh_source_kernel", "solo_mixsh_write_kernel", "solo_fan_clear_kernel", "solo_fan_mark_kernel",
           "solo_fan_totals_kernel", "solo_send_scan_kernel", "solo_fan_pool_kernel", "solo_fan_records_kernel")


@pytest.fixture(scope="module")
def lib():
    return T.built_library()


def _declared(name):
    m = re.search(r"\bint32_t\s+%s\s*\(([^)]*)\)" % name, T.header_text())
    assert m, name
    return [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]


def test_mix_shared_declared_exported_bound(lib):
    args = _declared("solo_mix_shared")
    assert args == ["solo_batch_t *b", "const int16_t *d_pcm_in", "int32_t n", "int32_t n_packets", "const int32_t *d_room", "int32_t n_rooms",
                    "const int16_t *d_gain_q12", "int32_t max_speakers", "const uint8_t *d_keep", "const int32_t *d_slots", "int16_t *d_pcm_spk",
                    "int32_t *d_spk_list", "int32_t *d_spk_rows", "int16_t *d_pcm_room", "int32_t *d_room_list", "int32_t *d_source",
                    "int64_t *d_energy", "uint8_t *d_mixed", "solo_mix_shared_count_t *d_count", "void *hip_stream"]
    assert hasattr(lib, "solo_mix_shared") and "solo_mix_shared" in solo_amd.ABI_SYMBOLS
    f = solo_amd.load_library().solo_mix_shared
    assert f.restype is C.c_int32 and len(f.argtypes) == 20
    assert [i for i, t in enumerate(f.argtypes) if t is C.c_int32] == [2, 3, 5, 7]          # n, n_packets, n_rooms, max_speakers


def test_send_fanout_declared_exported_bound(lib):
    args = _declared("solo_send_fanout")
    assert args == ["solo_batch_t *b", "const uint8_t *d_bits", "const int16_t *d_nbytes", "int32_t n_src", "const int32_t *d_source",
                    "const int32_t *d_dst_stream", "int32_t n_dst", "const uint8_t *d_send", "int32_t n_packets", "const int32_t *d_seq_base",
                    "int32_t first_seq", "solo_arrival_t *d_records", "int32_t max_records", "uint8_t *d_payload", "int64_t payload_capacity",
                    "solo_send_count_t *d_count", "void *hip_stream"]
    assert hasattr(lib, "solo_send_fanout") and "solo_send_fanout" in solo_amd.ABI_SYMBOLS
    f = solo_amd.load_library().solo_send_fanout
    assert f.restype is C.c_int32 and len(f.argtypes) == 17
    assert [i for i, t in enumerate(f.argtypes) if t is C.c_int32] == [3, 6, 8, 10, 12] and f.argtypes[14] is C.c_int64


def test_count_struct_is_24_bytes_on_both_sides():
    m = re.search(r"typedef struct \{([^}]*)\}\s*solo_mix_shared_count_t;", T.header_text())
    assert m
    fields = re.findall(r"(int32_t|int64_t)\s+([^;]+);", m.group(1))
    names = [x.strip() for _, group in fields for x in group.split(",")]
    size = sum((4 if ty == "int32_t" else 8) * len(group.split(",")) for ty, group in fields)
    assert size == 24 == C.sizeof(solo_amd.solo_mix_shared_count_t)
    assert names == [f[0] for f in solo_amd.solo_mix_shared_count_t._fields_] == list(solo_amd.SoloBatch.MIX_SHARED_COUNT)
    assert solo_amd.solo_mix_shared_count_t.clipped.offset == 16


def test_null_handle_is_refused(lib):
    x = (C.c_int32 * 64)()
    p = C.cast(x, C.c_void_p)
    l = solo_amd.load_library()
    assert l.solo_mix_shared(None, p, 1, 1, p, 1, None, 3, None, None, p, p, p, p, p, p, None, None, p, None) == -1
    assert l.solo_send_fanout(None, p, p, 1, p, None, 1, None, 1, None, 0, p, 1, p, 1, p, None) == -1


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="no LLVM binutils on this box")
def test_kernels_use_no_scratch(lib):
    sys.path.insert(0, os.path.join(T.ROOT, "tools"))
    from kernel_resources import kernel_resources
    seen = kernel_resources(solo_amd.LIB_PATH)
    for frag in KERNELS:
        hits = [r for name, r in seen.items() if re.search(r"\d%s(?![a-z_])" % frag, name)]
        assert len(hits) == 1, (frag, len(hits))                  # rate-independent: compiled once
        assert hits[0]["scratch"] == 0, (frag, hits[0])
        if "lds" in hits[0] and frag in ("solo_mixsh_energy_kernel", "solo_mixsh_select_kernel", "solo_mixsh_write_kernel"):
            assert hits[0]["lds"] == 0, (frag, hits[0])           # nothing but registers bounds the waves per SIMD


def _binding(t):
    b = object.__new__(solo_amd.SoloBatch)
    b.torch, b.lib, b.h = t, T.NoLib(), None
    b.n_streams, b.slot, b.packet_samples, b.device = 8, 512, 640, t.device("cpu")
    return b


def test_python_checks_of_mix_shared_raise_before_the_library():
    t = pytest.importorskip("torch")
    b = _binding(t)
    pcm, room = T.FakeDev((8, 3, 640), t.int16), T.FakeDev((8,), t.int32)
    bad = [
        dict(pcm=T.FakeDev((8, 3, 1280), t.int16), room=room),
        dict(pcm=T.FakeDev((8, 3, 640), t.int16, cuda=False), room=room),
        dict(pcm=T.FakeDev((8, 3, 640), t.int16, contiguous=False), room=room),
        dict(pcm=T.FakeDev((8, 0, 640), t.int16), room=room),
        dict(pcm=pcm, room=T.FakeDev((7,), t.int32)),
        dict(pcm=pcm, room=T.FakeDev((8,), t.int64)),
        dict(pcm=pcm, room=room, gain=T.FakeDev((9,), t.int16)),
        dict(pcm=pcm, room=room, max_speakers=0),
        dict(pcm=pcm, room=room, max_speakers=65),
        dict(pcm=pcm, room=room, keep=T.FakeDev((8,), t.int8)),
        dict(pcm=pcm, room=room, keep=T.FakeDev((8, 3), t.uint8)),
        dict(pcm=pcm, room=room, slots=T.FakeDev((8,), t.int64)),
        dict(pcm=pcm, room=room, slots=T.FakeDev((7,), t.int32)),
        dict(pcm=pcm, room=room, n_rooms=0),
        dict(pcm=pcm, room=room, n_rooms=9),
        dict(pcm=pcm, room=room, energy=T.FakeDev((8, 4), t.int64)),
        dict(pcm=pcm, room=room, mixed=T.FakeDev((8, 3), t.int8)),
        dict(pcm=pcm, room=room, pcm_spk=T.FakeDev((7, 3, 640), t.int16)),
        dict(pcm=pcm, room=room, n_rooms=4, pcm_room=T.FakeDev((8, 3, 640), t.int16)),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            b.mix_shared(**kw)


def test_python_checks_of_send_fanout_raise_before_the_library():
    t = pytest.importorskip("torch")
    b = _binding(t)
    bits, nb, src = T.FakeDev((6, 3, 512), t.uint8), T.FakeDev((6, 3, 2), t.int16), T.FakeDev((9,), t.int32)
    bad = [
        dict(bits=T.FakeDev((6, 3, 256), t.uint8), nbytes=nb, source=src),
        dict(bits=T.FakeDev((6, 3, 512), t.int8), nbytes=nb, source=src),
        dict(bits=T.FakeDev((6, 0, 512), t.uint8), nbytes=T.FakeDev((6, 0, 2), t.int16), source=src),
        dict(bits=bits, nbytes=T.FakeDev((9, 3, 2), t.int16), source=src),
        dict(bits=bits, nbytes=nb, source=T.FakeDev((9,), t.int64)),
        dict(bits=bits, nbytes=nb, source=T.FakeDev((0,), t.int32)),
        dict(bits=bits, nbytes=nb, source=T.FakeDev((9, 1), t.int32)),
        dict(bits=bits, nbytes=nb, source=src, dst_stream=T.FakeDev((6,), t.int32)),
        dict(bits=bits, nbytes=nb, source=src, send=T.FakeDev((6, 3), t.uint8)),
        dict(bits=bits, nbytes=nb, source=src, seq_base=T.FakeDev((9,), t.int16)),
        dict(bits=bits, nbytes=nb, source=src, first_seq=2 ** 31),
        dict(bits=bits, nbytes=nb, source=src, records=T.FakeDev((10, 4), t.int32)),
        dict(bits=bits, nbytes=nb, source=src, payload=T.FakeDev((10, 2), t.uint8)),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            b.send_fanout(**kw)


def test_signatures():
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(solo_amd.SoloBatch.mix_shared)[:7] == ["self", "pcm", "room", "gain", "max_speakers", "keep", "slots"]
    assert inspect.signature(solo_amd.SoloBatch.mix_shared).parameters["max_speakers"].default == 3
    assert sig(solo_amd.SoloBatch.mix_shared_count) == ["self", "count"]
    assert sig(solo_amd.SoloBatch.send_fanout) == ["self", "bits", "nbytes", "source", "dst_stream", "send", "first_seq", "seq_base", "records", "payload"]

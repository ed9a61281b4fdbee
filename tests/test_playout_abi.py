"""solo_playout_* (include/solo_mi355x.h): the symbols are declared, exported and bound; the parameter and count structures have the same
size in the header, in solo_playout.h (through the host build of tests/playout_host.cpp) and in the binding; the argument checks of
solo_amd.Playout raise before anything reaches the library; the new kernels exist once each and use no scratch.  No GPU call is made here."""
import ctypes as C
import inspect
import os
import re
import sys

import pytest

import playout_lib as PL
import playout_model as PM
import solo_amd
import solo_testlib as T

SYMBOLS = ("solo_playout_create", "solo_playout_destroy", "solo_playout_reset", "solo_playout_reset_rows", "solo_playout_get_state",
           "solo_playout_set_state", "solo_playout_plan", "solo_playout_gather", "solo_playout_render", "solo_playout_tick")
KERNELS = ("solo_playout_plan_kernel", "solo_playout_compact_kernel", "solo_playout_gather_kernel", "solo_playout_render_kernel",
           "solo_playout_count_kernel", "solo_rows_reset_kernel", "solo_rows_reset_all_kernel", "solo_rows_copy_kernel")


@pytest.fixture(scope="module")
def host():
    return PL.build_host()


def _struct_fields(name):
    m = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % name, T.header_text())
    assert m, name
    return [x.strip() for _, group in re.findall(r"(int32_t)\s+([^;]+);", m.group(1)) for x in group.split(",")]


def test_symbols_and_layouts(host):
    lib, loaded = T.built_library(), solo_amd.load_library()
    for s in SYMBOLS:
        assert s in solo_amd.ABI_SYMBOLS and hasattr(lib, s), s
        assert re.search(r"\b%s\s*\(" % s, T.header_text()), s
        assert getattr(loaded, s).argtypes is not None, s
    assert loaded.solo_playout_create.restype is C.c_void_p
    assert [len(getattr(loaded, s).argtypes) for s in SYMBOLS] == [2, 1, 2, 4, 5, 5, 12, 7, 22, 10]
    assert _struct_fields("solo_playout_params_t") == [f[0] for f in solo_amd.solo_playout_params_t._fields_] == list(PM.PARAMS)
    assert _struct_fields("solo_playout_plan_count_t") == [f[0] for f in solo_amd.solo_playout_plan_count_t._fields_] == ["n_one", "n_two", "n_stretch", "listed"]
    assert _struct_fields("solo_playout_render_count_t") == [f[0] for f in solo_amd.solo_playout_render_count_t._fields_] == list(PM.OUTCOMES)
    assert C.sizeof(solo_amd.solo_playout_params_t) == host.emu_po_params_size() == 32
    assert C.sizeof(solo_amd.solo_playout_plan_count_t) == host.emu_po_plan_count_size() == 16
    assert C.sizeof(solo_amd.solo_playout_render_count_t) == host.emu_po_render_count_size() == 32
    assert C.sizeof(solo_amd.solo_playout_count_t) == host.emu_po_count_size() == 48 and solo_amd.solo_playout_count_t.render.offset == 16
    assert solo_amd.PLAYOUT_STATE_BYTES == host.emu_po_state_bytes() == 128 and "#define SOLO_PLAYOUT_STATE_BYTES 128" in T.header_text()
    for o, name in enumerate(PM.OUTCOMES):                  # the outcome codes: header, binding and model agree
        assert "#define SOLO_PLAYOUT_%s %d\n" % (name.upper(), o) in T.header_text()
        assert solo_amd.Playout.OUTCOMES[o] == name.upper()
    assert solo_amd.Playout.ACTIONS == ("IDLE", "NORMAL", "HELD", "STRETCH", "ACCEL", "ACCEL_FORCED")
    assert solo_amd.Playout.PARAMS == PM.DEFAULTS


def test_null_objects_are_refused():
    lib = solo_amd.load_library()
    x = (C.c_int32 * 256)()
    a = C.c_void_p((C.addressof(x) + 15) & ~15)
    prm = solo_amd.Playout.params()
    assert lib.solo_playout_create(0, 640) is None and lib.solo_playout_create(4, 0) is None and lib.solo_playout_create(4, 324) is None
    assert lib.solo_playout_create(4, 1928) is None and lib.solo_playout_create(-1, 640) is None
    lib.solo_playout_destroy(None)
    assert lib.solo_playout_reset(None, None) == -1 and lib.solo_playout_reset_rows(None, a, 1, None) == -1
    assert lib.solo_playout_get_state(None, None, 1, a, None) == -1 and lib.solo_playout_set_state(None, None, 1, a, None) == -1
    assert lib.solo_playout_plan(None, a, None, 4, 8, C.byref(prm), a, a, a, a, a, None) == -1
    assert lib.solo_playout_gather(None, a, 4, a, 1, a, None) == -1
    assert lib.solo_playout_render(None, None, 4, C.byref(prm), 80, a, 0, 0, 0, *([None] * 8), a, a, a, a, None) == -1
    assert lib.solo_playout_tick(None, None, None, 4, C.byref(prm), a, a, a, a, None) == -1


def _fake_playout(t, n_rows=8, L=640):
    po = object.__new__(solo_amd.Playout)
    po.torch, po.lib, po.h, po.n_rows, po.packet_samples, po.device = t, T.NoLib(), None, n_rows, L, t.device("cpu")
    return po


def test_python_checks_raise_before_the_library():
    t = pytest.importorskip("torch")
    po = _fake_playout(t)
    F = T.FakeDev
    for bad in (dict(window=0), dict(window=33), dict(tolerate=4), dict(tolerate=-1), dict(lo=3, hi=2), dict(hi=65), dict(lo=-1), dict(cooldown=1001),
                dict(cooldown=-1), dict(start_ready=0), dict(max_span=-1), dict(cost_gate=2 ** 31), dict(lo=1.5), dict(speed=3)):
        with pytest.raises(ValueError):
            solo_amd.Playout.params(**bad)
    p = solo_amd.Playout.params(window=32, tolerate=3, lo=0, hi=64, cooldown=0, cost_gate=-1)
    assert (p.window, p.tolerate, p.lo, p.hi, p.cooldown, p.cost_gate, p.start_ready, p.max_span) == (32, 3, 0, 64, 0, -1, 2, 0)
    rep = F((8, 16), t.int32)
    bad_plan = [dict(reports=F((8, 15), t.int32), depth=8), dict(reports=F((7, 16), t.int32), depth=8), dict(reports=F((8, 16), t.int64), depth=8),
                dict(reports=F((8, 16), t.int32, cuda=False), depth=8), dict(reports=F((8, 16), t.int32, contiguous=False), depth=8),
                dict(reports=rep, depth=0), dict(reports=rep, depth=4097), dict(reports=rep, depth=8, window=40),
                dict(reports=rep, depth=8, rows=F((3,), t.int32)),                                # 3 rows listed, 8 reports
                dict(reports=F((3, 16), t.int32), depth=8, rows=F((3,), t.int64)), dict(reports=F((9, 16), t.int32), depth=8, rows=F((9,), t.int32)),
                dict(reports=F((3, 16), t.int32), depth=8, rows=F((3, 1), t.int32))]
    for kw in bad_plan:
        with pytest.raises(ValueError):
            po.plan(**kw)
    for rows in ([3, 3], [4, 2], [-1], [8], []):                                                  # host lists: checked here, before any copy
        with pytest.raises(ValueError):
            po.plan(F((len(rows), 16), t.int32), 8, rows=rows)
    act = F((8,), t.int32)
    one = dict(pcm_one=F((4, 640), t.int16), status_one=F((4,), t.int32))
    two = dict(pcm_two=F((2, 2, 640), t.int16), status_two=F((2,), t.int32), ts_accel=F((2, 1, 640), t.int16), cost_accel=F((2, 8), t.int32))
    st = dict(ts_stretch=F((1, 2, 640), t.int16), cost_stretch=F((1, 16), t.int32))
    bad_render = [dict(action=F((7,), t.int32), block_samples=80), dict(action=F((8,), t.int64), block_samples=80), dict(action=act, block_samples=0),
                  dict(action=act, block_samples=70), dict(action=act, block_samples=20),            # 32 blocks a packet
                  dict(action=act, block_samples=80, pcm_one=one["pcm_one"]), dict(action=act, block_samples=80, status_one=one["status_one"]),
                  dict(action=act, block_samples=80, pcm_one=F((4, 320), t.int16), status_one=one["status_one"]),
                  dict(action=act, block_samples=80, **dict(one, status_one=F((5,), t.int32))),
                  dict(action=act, block_samples=80, **dict(two, cost_accel=F((2, 16), t.int32))), dict(action=act, block_samples=80, **dict(two, ts_accel=None)),
                  dict(action=act, block_samples=80, **dict(two, pcm_two=F((2, 1, 640), t.int16))),
                  dict(action=act, block_samples=80, **st),                                           # a STRETCH row without a one-packet list
                  dict(action=act, block_samples=80, **dict(one, **dict(st, cost_stretch=F((1, 8), t.int32)))),
                  dict(action=act, block_samples=80, pcm_one=F((7, 640), t.int16), status_one=F((7,), t.int32), **two),   # 7 + 2 > 8 rows
                  dict(action=act, block_samples=80, cooldown=2000), dict(action=act, block_samples=80, rows=F((3,), t.int32))]
    for kw in bad_render:
        with pytest.raises(ValueError):
            po.render(**kw)
    for kw in (dict(pcm_one=F((4, 320), t.int16), stretch_pos=F((4,), t.int32), n_stretch=1), dict(pcm_one=F((4, 640), t.int16), stretch_pos=F((4,), t.int64), n_stretch=1),
               dict(pcm_one=F((4, 640), t.int16), stretch_pos=F((4,), t.int32), n_stretch=0), dict(pcm_one=F((4, 640), t.int16), stretch_pos=F((4,), t.int32), n_stretch=5),
               dict(pcm_one=F((9, 640), t.int16), stretch_pos=F((4,), t.int32), n_stretch=1)):
        with pytest.raises(ValueError):
            po.gather(**kw)
    with pytest.raises(ValueError):
        po.tick(object())                                                                         # not a SoloBatch
    b = object.__new__(solo_amd.SoloBatch)
    b.h, b.lib = None, T.NoLib()
    for n_streams, L in ((9, 640), (8, 1280)):
        b.n_streams, b.packet_samples = n_streams, L
        with pytest.raises(ValueError):
            po.tick(b)
    b.n_streams, b.packet_samples = 8, 640
    for kw in (dict(streams=[2, 2]), dict(streams=[8]), dict(streams=F((9,), t.int32)), dict(streams=F((2,), t.int16)), dict(hi=70), dict(gate=3)):
        with pytest.raises(ValueError):
            po.tick(b, **kw)
    for rows in ([1, 1], [8], [-1], [], list(range(9))):
        with pytest.raises(ValueError):
            po.reset_rows(rows)
    for kw in (dict(blob=F((8, 128), t.uint8)), dict(blob=F((8, 128 + 1280), t.int8)), dict(blob=F((9, 128 + 1280), t.uint8)), dict(blob=F((0, 128 + 1280), t.uint8)),
               dict(blob=F((3, 128 + 1280), t.uint8), rows=F((4,), t.int32)), dict(blob=F((2, 128 + 1280), t.uint8), rows=[1, 0])):
        with pytest.raises(ValueError):
            po.set_state(**kw)
    with pytest.raises(ValueError):
        po.get_state(rows=[3, 1])
    with pytest.raises(ValueError):
        po.count(F((5,), t.int32))
    assert po.state_bytes == 128 + 1280
    for n_rows, L in ((0, 640), (4, 0), (4, 644), (4, 1928)):
        with pytest.raises(ValueError):
            solo_amd.Playout(n_rows, L)


def test_signatures():
    P = solo_amd.Playout
    assert list(inspect.signature(P.tick).parameters) == ["self", "batch", "streams", "params"]
    assert list(inspect.signature(P.plan).parameters) == ["self", "reports", "depth", "rows", "params"]
    assert list(inspect.signature(P.render).parameters)[:3] == ["self", "action", "block_samples"]
    for name in ("reset", "reset_rows", "get_state", "set_state", "count", "gather"):
        assert callable(getattr(P, name)), name


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="no LLVM binutils on this box")
def test_playout_kernels_use_no_scratch():
    T.built_library()
    sys.path.insert(0, os.path.join(T.ROOT, "tools"))
    from kernel_resources import kernel_resources
    seen = kernel_resources(solo_amd.LIB_PATH)
    for frag in KERNELS:
        hits = [r for name, r in seen.items() if re.search(r"\d%s(?![a-z_])" % frag, name)]
        assert len(hits) == 1, (frag, len(hits))                  # rate-independent: compiled once
        assert hits[0]["scratch"] == 0, (frag, hits[0])

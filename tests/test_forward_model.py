"""Forwarding without transcoding (solo_forward_levels / solo_forward_route, solo_amd/csrc/solo_forward.h) without a GPU: the passes are
compiled for the host by this test (tests/forward_host.cpp, through tests/host_build.py) and compared with the independent model of
tests/forward_model.py, record for record and state word for state word after every tick of the scenarios the GPU runs as well
(tests/test_gpu_forward.py); then the model's own properties, the argument rules, the ABI, the binding and the built library's kernels."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import forward_model as M
import solo_testlib as T
from host_build import host_lib

FORWARD_SYMBOLS = ("solo_forward_create", "solo_forward_destroy", "solo_forward_reset", "solo_forward_reset_rooms", "solo_forward_get_state",
                   "solo_forward_set_state", "solo_forward_levels", "solo_forward_route")
FILL8, FILL32 = 0xA5, -7


@pytest.fixture(scope="module")
def host():
    lib = host_lib("forward")
    lib.emu_forward_create.restype = C.c_void_p
    lib.emu_forward_create.argtypes = [C.c_int, C.c_int]
    lib.emu_forward_destroy.argtypes = [C.c_void_p]
    lib.emu_forward_reset_rooms.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    lib.emu_forward_state.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    lib.emu_forward_levels.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.emu_forward_route.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def p(x):
    return None if x is None else x.ctypes.data


def send_count_of(a):
    return dict(records=int(a[0]), records_needed=int(a[1]), bytes=int(a[2:4].view(np.int64)[0]), bytes_needed=int(a[4:6].view(np.int64)[0]),
                empty=int(a[6]), refused=int(a[7]))


class HostForward:
    """the host form's object; call() is what forward_model.run() drives"""

    def __init__(self, lib, n_rows, K):
        self.lib, self.n_rows, self.K = lib, n_rows, K
        self.h = lib.emu_forward_create(n_rows, K)
        assert self.h

    def state(self):
        w = np.zeros((self.n_rows, 4 * self.K), np.int32)
        self.lib.emu_forward_state(self.h, p(w), 0)
        return w

    def set_state(self, w):
        w = np.ascontiguousarray(w, np.int32)
        assert w.shape == (self.n_rows, 4 * self.K)
        self.lib.emu_forward_state(self.h, p(w), 1)

    def levels(self, tick, n):
        arr = tick["arrivals"]
        ri, sa, lv = np.full((n + 2, 4), FILL32, np.int32), np.full(n + 2, FILL8, np.uint8), np.full(n + 2, FILL8, np.uint8)
        assert self.lib.emu_forward_levels(p(arr), p(tick["level_in"]), arr.shape[0], n, tick["default_level"], p(ri), p(sa), p(lv)) == 0
        assert (ri[n:] == FILL32).all() and (sa[n:] == FILL8).all() and (lv[n:] == FILL8).all()
        return ri[:n].copy(), sa[:n], lv[:n]

    def route(self, tick, ri, n, n_rooms, mr, guard=8):
        arr = tick["arrivals"]
        rec, sc, cnt = np.full((mr + guard, 5), FILL32, np.int32), np.full(8, -9, np.int32), np.full(8, -9, np.int32)
        lf, src = np.full(n * self.K + guard, FILL8, np.uint8), np.full((n_rooms + 1, self.K), FILL32, np.int32)
        r = self.lib.emu_forward_route(self.h, p(arr), arr.shape[0], p(ri), p(tick["sel"]), p(tick["room"]), n, n_rooms, p(rec), mr, p(sc), p(lf), p(src), p(cnt))
        return r, rec, sc, cnt, lf, src

    def call(self, n, n_rooms):
        def go(tick, _words, mr):
            ri, sa, lv = self.levels(tick, n)
            r, rec, sc, cnt, lf, src = self.route(tick, ri, n, n_rooms, mr)
            assert r == 0
            assert (lf[n * self.K:] == FILL8).all() and (src[n_rooms:] == FILL32).all()
            return dict(rowinfo=ri, sa=sa, level=lv, records=rec, send_count=send_count_of(sc), count=dict(zip(M.COUNT_FIELDS, (int(v) for v in cnt))),
                        level_fwd=lf[:n * self.K].astype(np.int64), slot_src=src[:n_rooms], state=self.state(), fill32=FILL32, fill8=FILL8)
        return go

    def close(self):
        self.lib.emu_forward_destroy(self.h)


# ---- structure sizes, ABI -------------------------------------------------------------------------------------------------------------
def test_structure_sizes(host):
    import solo_amd
    assert host.emu_forward_sizes(0) == 16 == C.sizeof(solo_amd.solo_forward_row_t)
    assert host.emu_forward_sizes(1) == 32 == C.sizeof(solo_amd.solo_forward_count_t)
    assert host.emu_forward_sizes(2) == 16 and host.emu_forward_sizes(3) == 48
    assert solo_amd.solo_forward_row_t.byte.offset == 14 and solo_amd.solo_forward_count_t.switches.offset == 28
    assert [n for n, _ in solo_amd.solo_forward_count_t._fields_] == list(M.COUNT_FIELDS)
    assert [n for n, _ in solo_amd.solo_forward_row_t._fields_] == list(M.ROW_FIELDS)
    src = open(os.path.join(T.ROOT, "solo_amd", "csrc", "solo_forward.h")).read()
    assert "static_assert(sizeof(SxFwdRow) == 16" in src and "static_assert(sizeof(SxFwdCount) == 32" in src
    assert "typedef solo_forward_row_t SxFwdRow" in src and "typedef solo_forward_count_t SxFwdCount" in src       # each ABI record defined once
    assert "#define SOLO_FORWARD_STATE_BYTES(slots) (16 * (slots))" in T.header_text()


def test_symbols_declared_exported_and_bound():
    import solo_amd
    hdr = T.header_text()
    lib = T.built_library()
    for name in FORWARD_SYMBOLS:
        assert name in solo_amd.ABI_SYMBOLS and (name + "(") in hdr.replace(" (", "("), name
        assert hasattr(lib, name), name
    bound = solo_amd.load_library()
    assert len(bound.solo_forward_levels.argtypes) == 9 and len(bound.solo_forward_route.argtypes) == 15
    assert bound.solo_forward_create.restype is C.c_void_p and len(bound.solo_forward_reset_rooms.argtypes) == 4
    assert len(bound.solo_forward_get_state.argtypes) == 5 and len(bound.solo_forward_set_state.argtypes) == 5
    assert issubclass(solo_amd.Forward, solo_amd._RowStateObject)
    for m in ("levels", "route", "count", "reset", "get_state", "set_state", "close"):
        assert callable(getattr(solo_amd.Forward, m)), m


def test_capture_claims_name_a_test():
    """the header calls solo_forward_levels and solo_forward_route capturable: tests/test_gpu_forward.py names the test that captures each
    (its module loads without a GPU), as tests/test_gpu_graph_replay.py does for the calls of its table"""
    import ast
    import re
    import test_gpu_forward as GPU
    m = re.search(r"/\* Forwarding without transcoding.*?\*/", open(os.path.join(T.ROOT, "include", "solo_mi355x.h")).read(), flags=re.S)
    assert m and m.group(0).count("capturable") == 2 and "solo_forward_levels" in m.group(0) and "solo_forward_route" in m.group(0)
    tests = {n.name for n in ast.parse(open(GPU.__file__).read()).body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}
    assert set(GPU.CAPTURED) == {"solo_forward_levels", "solo_forward_route"} and set(GPU.CAPTURED.values()) <= tests
    for name in GPU.CAPTURED.values():
        assert name in m.group(0), name                             # ... and the header names it


# ---- levels -----------------------------------------------------------------------------------------------------------------------------
def test_level_rules_by_hand():
    arr = np.array([(0, 7, 0, 0, 9), (0, 5, 1, 0, 9), (0, 6, -1, 0, 9), (1, 3, 0, 0, 9), (-1, 0, 0, 0, 0), (4, 9, 0, 0, 9), (2, 8, 0, 0, 9), (2, 8, 1, 0, 9)], np.int32)
    lev = np.array([0x80 | 30, 20, 0x80 | 1, 255, 3, 3, 0x80 | 40, 40], np.uint8)
    rows = M.levels(arr, lev, 4, 255)
    assert rows[0] == dict(min_seq=5, max_seq=7, dgrams=2, sa=0, level=20, byte=20, pad=0)                # desc -1 does not count; the loudest
    assert rows[1] == dict(min_seq=3, max_seq=3, dgrams=1, sa=0, level=127, byte=0x7F, pad=0)             # a datagram without a byte
    assert rows[2] == dict(min_seq=8, max_seq=8, dgrams=2, sa=255, level=40, byte=0x80 | 40, pad=0)       # voiced before unvoiced
    assert rows[3] == dict(min_seq=-1, max_seq=-1, dgrams=0, sa=0, level=127, byte=0x7F, pad=0)
    assert M.levels(arr, lev, 4, 0x80 | 9)[1]["byte"] == 0x80 | 9 and M.levels(arr, None, 4, 33)[0]["byte"] == 33
    assert M.levels(arr, None, 4, 255)[0]["byte"] == 0x7F


@pytest.mark.parametrize("seed", [1, 2])
def test_host_levels_against_model(host, seed):
    rng = np.random.default_rng(seed)
    n, nd = 37, 600
    arr = np.stack([rng.integers(-2, n + 2, nd), rng.integers(0, 2 ** 31, nd), rng.integers(-1, 3, nd), rng.integers(0, 999, nd), rng.integers(1, 99, nd)], 1).astype(np.int32)
    arr[arr[:, 0] == 5, 0] = 6                                     # a row without arrivals
    lev = rng.integers(0, 256, nd).astype(np.uint8)
    lev[rng.integers(0, 3, nd) == 0] = 255
    f = HostForward(host, n, 2)
    for level_in, default in ((lev, 255), (lev, 0x80 | 77), (None, 12), (None, 255)):
        tick = dict(arrivals=arr, level_in=level_in, default_level=default)
        ri, sa, lv = f.levels(tick, n)
        rows = M.levels(arr, level_in, n, default)
        assert np.array_equal(ri, M.rowinfo_words(rows)) and M.rowinfo_of_words(ri) == rows
        assert sa.tolist() == [r["sa"] for r in rows] and lv.tolist() == [r["level"] for r in rows]
        assert rows[5]["dgrams"] == 0 and rows[5]["min_seq"] == -1
    empty = dict(arrivals=np.zeros((0, 5), np.int32), level_in=None, default_level=3)
    ri, sa, lv = f.levels(empty, n)
    assert np.array_equal(ri, M.rowinfo_words(M.levels(empty["arrivals"], None, n, 3))) and (lv == 127).all() and (sa == 0).all()
    f.close()


# ---- the scenarios: model against emulation ------------------------------------------------------------------------------------------------
def check_model_properties(results, K, n_rooms):
    """what the scenarios must have hit, and what the model must keep"""
    total = {k: sum(r["count"][k] for r in results) for k in M.COUNT_FIELDS}
    switched, prev = set(), [[-1] * K for _ in range(n_rooms)]
    owner, last_src, top = {}, {}, {}
    for res in results:
        for r in range(n_rooms):
            for k in range(K):
                if res["slot_src"][r][k] not in (-1, prev[r][k]):
                    switched.add(k)
            prev[r] = list(res["slot_src"][r])
        by_slot = {}
        for r, k, q, src in res["forwarded"]:
            assert owner.setdefault((r, k, q), src) == src, ("two sources share a packet number of a slot", r, k, q)
            by_slot.setdefault((r, k), []).append((q, src))
        for slot, qs in by_slot.items():
            assert len({s for _, s in qs}) == 1                     # one source per slot and call
            if last_src.get(slot) != qs[0][1] and slot in top:
                assert min(q for q, _ in qs) > top[slot], ("a slot's packet numbers went back across a switch", slot)
            last_src[slot] = qs[0][1]
            top[slot] = max(top.get(slot, -1), max(q for q, _ in qs))
    return total, switched


@pytest.mark.parametrize("K", [2, 3])
def test_scenario_a_host_against_model(host, K):
    n, n_rooms = M.A_ROWS, M.A_ROOMS
    ticks = M.scenario_a(100 + K, K)
    assert len(ticks) == 12 and {t["cut"] for t in ticks} == {"all", "mid", "zero"}
    f, model = HostForward(host, n, K), M.Forward(n, K)
    results = M.run(model, ticks, n, n_rooms, f.call(n, n_rooms))
    total, switched = check_model_properties(results, K, n_rooms)
    assert all(total[k] > 0 for k in M.COUNT_FIELDS), total          # a generator that never produces `stale` fails here
    assert switched == set(range(K)), switched
    sizes = {tuple(sorted(np.bincount(t["room"][t["room"] >= 0]).tolist())) for t in ticks}
    assert sizes == {(1, 2, 3, 5, 12), (1, 2, 3, 4, 13)} and all(t["room"][23] == -1 for t in ticks)
    assert any(max(q for _, _, q, _ in r["forwarded"]) >= M.TOP - 2 for r in results if r["forwarded"])          # a packet number near 2^31
    # the same ticks with the arrivals in another order: the same state, counts and per-row outputs, the same records as a multiset
    rng = np.random.default_rng(7)
    f2, model2 = HostForward(host, n, K), M.Forward(n, K)
    again = M.run(model2, [M.permuted(t, rng) for t in ticks], n, n_rooms, f2.call(n, n_rooms), cut_all=True)
    for a, b in zip(results, again):
        assert a["count"] == b["count"] and a["slot_src"] == b["slot_src"] and a["level_fwd"] == b["level_fwd"]
        assert sorted(a["records"]) == sorted(b["records"])
    assert np.array_equal(model.state(), model2.state()) and np.array_equal(f.state(), f2.state())
    f.close()
    f2.close()


def test_scenario_b_host_against_model(host):
    n, K = M.B_ROWS, 3
    ticks = M.scenario_b(5)
    f, model = HostForward(host, n, K), M.Forward(n, K)
    results = M.run(model, ticks, n, 1, f.call(n, 1))
    total, switched = check_model_properties(results, K, 1)
    assert total["forwarded"] > 0 and total["no_slot"] > 0 and total["not_selected"] > 0 and switched == {0, 1, 2}
    assert all(len(r["records"]) == 699 * r["count"]["forwarded"] for r in results)
    rng = np.random.default_rng(8)
    f2, model2 = HostForward(host, n, K), M.Forward(n, K)
    again = M.run(model2, [M.permuted(t, rng) for t in ticks], n, 1, f2.call(n, 1), cut_all=True)
    assert all(sorted(a["records"]) == sorted(b["records"]) and a["count"] == b["count"] for a, b in zip(results, again))
    assert np.array_equal(f.state(), f2.state())
    f.close()
    f2.close()


def test_refused_room_id_and_control_plane(host):
    n, K = M.A_ROWS, 3
    ticks = M.scenario_a(3, K)
    f, model = HostForward(host, n, K), M.Forward(n, K)
    M.run(model, ticks[:3], n, M.A_ROOMS, f.call(n, M.A_ROOMS))
    before = f.state()
    assert not np.array_equal(before, M.Forward(n, K).state())
    for bad in (-2, M.A_ROOMS):
        tick = dict(ticks[3], room=ticks[3]["room"].copy())
        tick["room"][9] = bad
        ri, _, _ = f.levels(tick, n)
        r, rec, sc, cnt, lf, src = f.route(tick, ri, n, M.A_ROOMS, 50)
        assert r == 1 and cnt[0] == -1 and sc[0] == -1 and (cnt[1:] == -9).all() and (sc[1:] == -9).all()
        assert (rec == FILL32).all() and (lf == FILL8).all() and (src == FILL32).all() and np.array_equal(f.state(), before)
        assert model.route(tick["arrivals"], M.rowinfo_of_words(ri), tick["sel"], tick["room"], n, M.A_ROOMS) is None
        assert np.array_equal(model.state(), before)
    # the listed reset: a HOST list, inside [0, n_rows), none twice
    for lst in ([], [n], [-1], [2, 2]):
        a = np.array(lst, np.int32)
        assert host.emu_forward_reset_rooms(f.h, p(a) if lst else None, len(lst)) == -1
    assert np.array_equal(f.state(), before)
    a = np.array([4, 1], np.int32)
    assert host.emu_forward_reset_rooms(f.h, p(a), 2) == 0
    model.reset([4, 1])
    assert np.array_equal(f.state(), model.state()) and f.state()[4].tolist() == [-1, 0, 0, 0] * K and np.array_equal(f.state()[2], before[2])
    # a state that travels: the rest of the scenario on a second object equals the model
    g = HostForward(host, n, K)
    g.set_state(f.state())
    M.run(model, ticks[3:], n, M.A_ROOMS, g.call(n, M.A_ROOMS))
    f.close()
    g.close()


def test_argument_rules(host):
    """what returns -1 with nothing done: sx_fwd_levels_ok and sx_fwd_route_ok, the checks solo_api.hip makes"""
    n, K = 8, 2
    assert not host.emu_forward_create(0, 2) and not host.emu_forward_create(4, 0) and not host.emu_forward_create(4, 9)
    f = HostForward(host, n, K)
    arr = np.zeros((4, 5), np.int32)
    ri, sa, lv = np.zeros((n, 4), np.int32), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    ok = [p(arr), None, 4, n, 255, p(ri), p(sa), p(lv)]
    assert host.emu_forward_levels(*ok) == 0
    for at, v in ((5, None), (6, None), (7, None), (2, -1), (0, None), (3, 0), (3, -1), (4, -1), (4, 256), (5, p(ri) + 2), (0, p(arr) + 1)):
        bad = list(ok)
        bad[at] = v
        assert host.emu_forward_levels(*bad) == -1, (at, v)
    assert host.emu_forward_levels(None, None, 0, n, 0, p(ri), p(sa), p(lv)) == 0
    sel, room = np.ones(n, np.uint8), np.zeros(n, np.int32)
    rec, sc, cnt = np.zeros((64, 5), np.int32), np.zeros(4, np.int64).view(np.int32), np.zeros(8, np.int32)
    lf, src = np.zeros(n * K, np.uint8), np.zeros((n, K), np.int32)
    ok = [f.h, p(arr), 4, p(ri), p(sel), p(room), n, 1, p(rec), 64, p(sc), p(lf), p(src), p(cnt)]
    state = f.state()
    assert host.emu_forward_route(*ok) == 0
    f.set_state(state)
    for at, v in ((0, None), (3, None), (4, None), (5, None), (8, None), (10, None), (13, None), (6, 0), (6, n + 1), (7, 0), (7, n + 1), (2, -1), (1, None),
                  (9, -1), (1, p(arr) + 2), (3, p(ri) + 1), (5, p(room) + 2), (8, p(rec) + 2), (12, p(src) + 2), (13, p(cnt) + 2), (10, p(sc) + 4)):
        bad = list(ok)
        bad[at] = v
        assert host.emu_forward_route(*bad) == -1, (at, v)
    assert np.array_equal(f.state(), state)
    bad = list(ok)
    bad[2] = 2 ** 31 // (n - 1) + 1                                # n_dgrams x (n - 1) >= 2^31 (refused before anything is read)
    assert host.emu_forward_route(*bad) == -1
    ok[11] = ok[12] = None                                         # d_level_fwd and d_slot_src are optional; no arrivals at all
    ok[1], ok[2] = None, 0
    assert host.emu_forward_route(*ok) == 0
    f.close()


# ---- the Python binding refuses bad arguments before the library ------------------------------------------------------------------------
def test_binding_checks():
    import solo_amd
    torch = pytest.importorskip("torch")
    for args in ((0, 3), (4, 0), (4, 9)):
        with pytest.raises(ValueError):
            solo_amd.Forward(*args)
    o = object.__new__(solo_amd.Forward)
    o.n_rows, o.slots, o.state_bytes = 8, 3, 48
    o.torch, o.lib, o.h, o.device = torch, T.NoLib(), None, torch.device("cpu")
    o._stream = lambda: None
    D = T.FakeDev
    I32, U8 = torch.int32, torch.uint8
    good = dict(arrivals=D((10, 5), I32), level_in=D((10,), U8))
    for over in (dict(arrivals=D((10, 4), I32)), dict(arrivals=D((10, 5), I32, cuda=False)), dict(level_in=D((9,), U8)), dict(level_in=D((10,), I32)),
                 dict(default_level=256), dict(default_level=-1), dict(n_rows=0)):
        with pytest.raises(ValueError):
            o.levels(**dict(good, **over))
    good = dict(arrivals=D((10, 5), I32), rowinfo=D((8, 4), I32), sel=D((8,), U8), room=D((8,), I32), n_rooms=2)
    for over in (dict(arrivals=D((10, 3), I32)), dict(rowinfo=D((9, 4), I32)), dict(rowinfo=D((8, 3), I32)), dict(sel=D((7,), U8)), dict(sel=D((8,), I32)),
                 dict(room=D((7,), I32)), dict(room=D((8,), I32, contiguous=False)), dict(n_rooms=0), dict(n_rooms=9), dict(max_records=-1),
                 dict(records=D((10, 4), I32)), dict(arrivals=D((2 ** 31 // 7 + 1, 5), I32))):
        with pytest.raises(ValueError):
            o.route(**dict(good, **over))
    for lst in ([], [8], [0, 0]):
        with pytest.raises(ValueError):
            o.reset(lst)

    class Recorder:
        calls = []

        def __getattr__(self, name):
            return lambda *a: self.calls.append((name,) + tuple(tuple(x) if isinstance(x, C.Array) else x for x in a)) or 0
    o.lib, o.h = Recorder(), 0x77
    o.reset()
    o.reset([5, 2])
    assert Recorder.calls == [("solo_forward_reset", 0x77, None), ("solo_forward_reset_rooms", 0x77, (5, 2), 2, None)]


# ---- the built library's kernels ------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="no LLVM binutils on this box")
def test_forward_kernels_use_no_scratch():
    """no private memory in any kernel of the stage: read from each kernel's resource record, nothing else"""
    import solo_amd
    T.built_library()
    sys.path.insert(0, os.path.join(T.ROOT, "tools"))
    from kernel_resources import kernel_resources
    seen = kernel_resources(solo_amd.LIB_PATH)
    for frag in ("solo_forward_levels_clear_kernel", "solo_forward_levels_kernel", "solo_forward_levels_finish_kernel", "solo_forward_begin_kernel",
                 "solo_forward_rooms_kernel", "solo_forward_verdicts_kernel", "solo_forward_scan_kernel", "solo_forward_emit_kernel"):
        hits = [r for name, r in seen.items() if frag in name]
        assert len(hits) == 1, (frag, len(hits))                  # rate-independent: compiled once
        assert hits[0]["scratch"] == 0, (frag, hits[0])
    assert len([name for name in seen if "solo_forward_" in name]) == 8

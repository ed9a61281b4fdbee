"""Read side of the receiver ring (solo_recv_report, solo_amd/csrc/solo_recv_report.h) without a GPU: the per-stream queue scan, the
selection rule, the record layout and the play-out classification are compiled for the host by this test (tests/recv_report_host.cpp,
through tests/host_build.py) and compared with the independent model of tests/recv_report_model.py on random rings -- every depth
around the group sizes of the kernel, play-out positions that make the window wrap the ring, empty / full / head-missing /
only-last-entry queues, every branch of the selection; the built library's new kernels use no scratch."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import solo_testlib as T
from host_build import host_lib
from recv_report_model import FIELDS, RingModel, lens_words, queue_fields, selected

DEPTHS = [1, 2, 5, 8, 63, 64, 65, 4096]


@pytest.fixture(scope="module")
def host():
    lib = host_lib("recv_report")
    lib.emu_recv_report.argtypes = [C.c_void_p] * 5 + [C.c_int] * 5 + [C.c_void_p] * 4
    lib.emu_recv_play_class.argtypes = [C.c_uint]
    return lib


def test_struct_sizes(host):
    import solo_amd
    assert host.emu_recv_report_size() == 64 == C.sizeof(solo_amd.solo_recv_report_t)
    assert host.emu_recv_report_count_size() == 8 == C.sizeof(solo_amd.solo_recv_report_count_t)
    assert host.emu_recv_trk_words() == 10 == len(FIELDS) - 6


def test_group_sizes(host):
    for d in range(1, 200):
        g = host.emu_recv_group(d)
        assert g in (1, 2, 4, 8, 16, 32, 64) and g >= min(d, 64) and (g == 1 or g // 2 < min(d, 64)), (d, g)
    assert host.emu_recv_group(4096) == 64


def test_play_class(host):
    for la in (0, 1, 77, 0x7FFF):
        for lb in (0, 1, 8, 0x7FFF):
            want = 0 if la and lb else 1 if la else 2 if lb else 3
            assert host.emu_recv_play_class(la | (lb << 16)) == want


def test_selection_rule(host):
    for depth in (1, 8, 65):
        for ready in range(0, depth + 1):
            for span in {0, ready, depth}:
                for m in (-3, 0, 1, ready, ready + 1, depth, depth + 1):
                    for max_span in (-1, 0, 1, span, span + 1, depth):
                        assert bool(host.emu_recv_select(ready, span, m, max_span)) == bool(selected(ready, span, m, max_span)), (ready, span, m, max_span)


def _random_queue(rng, kind, play, depth):
    """{seq: [lenA, lenB]} inside [play, play + depth)"""
    ln = lambda: int(rng.integers(1, 0x8000))
    one = lambda: [[ln(), 0], [0, ln()], [ln(), ln()]][int(rng.integers(0, 3))]
    if kind == "empty":
        return {}
    if kind == "full":
        return {play + k: one() for k in range(depth)}
    if kind == "last":
        return {play + depth - 1: one()}
    if kind == "first":
        return {play: one()}
    fill = float(rng.random())
    q = {play + k: one() for k in range(depth) if rng.random() < fill}
    if kind == "nohead":
        q.pop(play, None)
    if kind == "run":                                          # a run from the head, a hole, then something behind it
        k0 = int(rng.integers(0, depth + 1))
        q = {play + k: one() for k in range(k0)}
        if k0 + 1 < depth:
            q[play + int(rng.integers(k0 + 1, depth))] = one()
    return q


def _run_host(host, lens, play, trk, streams, min_ready, max_span, clear, depth):
    n = len(streams) if streams is not None else len(play)
    FILL = 0x5A5A5A5A
    rep = np.full((n + 2, 16), FILL, np.uint32)
    sel = np.zeros(n, np.int32)
    lst, rows = np.full(n + 2, -7, np.int32), np.full(n + 2, -7, np.int32)
    p = lambda x: x.ctypes.data if x is not None else None
    mv = None if isinstance(min_ready, int) else np.asarray(min_ready, np.int32)
    k = host.emu_recv_report(p(lens), p(play), p(trk), p(streams), p(mv), n, depth, min_ready if mv is None else 0, max_span, int(clear), p(rep), p(sel), p(lst),
                             p(rows))
    assert (rep[n:] == FILL).all() and (lst[k:] == -7).all() and (rows[k:] == -7).all()
    return rep[:n].view(np.int32).astype(np.int64), lst[:k].tolist(), rows[:k].tolist()


@pytest.mark.parametrize("depth", DEPTHS)
def test_host_report_against_model(host, depth):
    rng = np.random.default_rng(4000 + depth)
    kinds = ["empty", "full", "last", "first", "nohead", "run", "random"]
    N = 70 if depth <= 65 else 21
    m = RingModel(N, depth, 0x7FFF)
    m.track(True)
    seen_wrap = 0
    for s in range(N):
        # play-out positions: 0, multiples of the depth, and positions whose window wraps the ring at every place
        m.play[s] = [0, depth, 3 * depth][s] if s < 3 else int(rng.integers(0, 5 * depth + 7))
        seen_wrap += (m.play[s] % depth) != 0
        m.q[s] = _random_queue(rng, kinds[s % len(kinds)], m.play[s], depth)
        m.cnt[s] = [int(x) for x in rng.integers(0, 2 ** 32, 9)]
        m.margin[s] = int(rng.integers(0, depth + 1))
    assert depth == 1 or seen_wrap >= N // 3                  # (at depth 2 every second position is a multiple of the depth)
    lens = lens_words(m.q, m.play, depth)
    play = np.array(m.play, np.int32)

    def trk_of(model):
        return np.array([list(c) + [mg] for c, mg in zip(model.cnt, model.margin)], np.uint32)

    subset = np.sort(rng.choice(N, N // 2, replace=False)).astype(np.int32)
    thresholds = [0, -1, 1, 2, depth // 2, depth - 1, depth, depth + 1]
    per_row = rng.integers(-1, depth + 2, N).astype(np.int32)
    outcomes = set()
    for streams in (None, subset):
        n = N if streams is None else len(streams)
        for mr in thresholds + [per_row[:n].copy()]:
            for max_span in (0, 1, depth // 2 + 1, depth):
                trk = trk_of(m)
                want_rep, want_lst, want_rows = m.report(None if streams is None else streams.tolist(), mr if isinstance(mr, int) else mr.tolist(), max_span)
                rep, lst, rows = _run_host(host, lens, play, trk, streams, mr, max_span, False, depth)
                assert np.array_equal(rep, _as_i32(want_rep)), (depth, mr, max_span)
                assert lst == want_lst and rows == want_rows, (depth, mr, max_span)
                assert np.array_equal(trk, trk_of(m))                                 # (nothing cleared without the flag)
                outcomes |= {("some", 0 < len(lst) < n), ("all", len(lst) == n), ("none", len(lst) == 0)}
    assert ("all", True) in outcomes and ("none", True) in outcomes and (depth == 1 or ("some", True) in outcomes)
    # without counters: zeros, margin = depth; the queue fields do not change
    rep, lst, rows = _run_host(host, lens, play, None, None, 1, 0, True, depth)
    assert np.array_equal(rep[:, :6], _as_i32(m.report()[0])[:, :6]) and (rep[:, 6:15] == 0).all() and (rep[:, 15] == depth).all()
    # the clear flag: the listed streams' margins go back to `depth` AFTER they were reported, the others stay
    trk = trk_of(m)
    before = trk.copy()
    rep, _, _ = _run_host(host, lens, play, trk, subset, 1, 0, True, depth)
    want_rep, _, _ = m.report(subset.tolist(), 1, 0, clear_margin=True)
    assert np.array_equal(rep, _as_i32(want_rep))
    assert np.array_equal(trk, trk_of(m)) and (trk[subset, 9] == depth).all()
    others = np.setdiff1d(np.arange(N), subset)
    assert np.array_equal(trk[others], before[others]) and np.array_equal(trk[:, :9], before[:, :9])


def _as_i32(rep):
    """the model's int64 table as the int32 words of the record (the counters are uint32)"""
    return (rep & 0xFFFFFFFF).astype(np.uint32).view(np.int32).astype(np.int64).reshape(rep.shape)


def test_queue_fields_of_the_model_on_known_queues():
    """the model itself, on queues whose fields are known by hand"""
    assert queue_fields({}, 5, 8) == (0, 0, 0, 0, 0)
    assert queue_fields({5: [10, 0]}, 5, 8) == (1, 0, 1, 1, 1)
    assert queue_fields({5: [0, 9], 6: [3, 4], 8: [1, 0]}, 5, 8) == (3, 1, 2, 4, 2)
    assert queue_fields({12: [1, 1]}, 5, 8) == (1, 1, 0, 8, 0)
    assert queue_fields({k: [1, 1] for k in range(5, 13)}, 5, 8) == (8, 8, 8, 8, 3)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="no LLVM binutils on this box")
def test_report_kernels_use_no_scratch_and_exist_in_both_builds():
    import solo_amd
    import __graft_entry__ as g
    if not (os.path.exists(solo_amd.LIB_PATH) and os.path.exists(g.LIB_ALT)):
        g.build()
    sys.path.insert(0, os.path.join(T.ROOT, "tools"))
    from kernel_resources import kernel_resources
    for lib in (solo_amd.LIB_PATH, g.LIB_ALT):
        seen = kernel_resources(lib)
        for frag in ("solo_recv_report_kernel", "solo_recv_compact_kernel", "solo_recv_account_kernel", "solo_recv_trk_reset_kernel",
                     "solo_recv_trk_reset_list_kernel"):
            hits = [r for name, r in seen.items() if frag in name]
            assert len(hits) == 1, (lib, frag, len(hits))             # rate-independent: compiled once
            assert hits[0]["scratch"] == 0, (lib, frag, hits[0])
        hits = [r for name, r in seen.items() if "solo_recv_insert_kernel" in name]
        assert len(hits) == 2, (lib, len(hits))                        # the insert kernel that counts per stream: both rates

"""Sender back end (solo_send_pack, solo_amd/csrc/solo_send.h) without a GPU: the length rules, the three passes and the byte copy are
compiled for the host by this test (tests/send_pack_host.cpp, through tests/host_build.py) and compared with the independent numpy
model of tests/send_pack_model.py on random length records; the wave scan's host form against a running sum; the built library's new
kernels use no scratch."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import solo_testlib as T
from host_build import host_lib
from send_pack_model import INT32_MAX, REASONS, model_pack


@pytest.fixture(scope="module")
def host():
    lib = host_lib("send_pack")
    lib.emu_send_plan.argtypes = [C.c_int] * 5 + [C.c_longlong, C.c_void_p]
    lib.emu_send_pack.argtypes = [C.c_void_p] * 5 + [C.c_int] * 5 + [C.c_void_p, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p]
    lib.emu_send_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    lib.emu_wave_scan.argtypes = [C.c_void_p]
    return lib


def test_count_struct_is_32_bytes(host):
    import solo_amd
    assert host.emu_send_count_size() == 32 == C.sizeof(solo_amd.solo_send_count_t)


def test_plan_rules(host):
    """the rule table of include/solo_mi355x.h, case by case: (total, n1, slot, hbb, mask, seq) -> (why, len0, len1)"""
    OK, EMPTY, LARGE, NEG, OVER, SHORT, SEQ = range(7)
    cases = [((80, 40, 512, 8, 3, 5), (OK, 40, 40)), ((80, 40, 512, 8, 1, 5), (OK, 40, 0)), ((80, 40, 512, 8, 2, 5), (OK, 0, 40)),
             ((80, 40, 512, 8, 0, 5), (OK, 0, 0)), ((0, 0, 512, 8, 3, 5), (EMPTY, 0, 0)), ((-3, 7, 512, 8, 3, -1), (EMPTY, 0, 0)),
             ((513, 40, 512, 8, 3, 5), (LARGE, 0, 0)), ((512, 40, 512, 8, 3, 5), (OK, 472, 40)), ((80, -1, 512, 8, 3, 5), (NEG, 0, 0)),
             ((80, 81, 512, 8, 3, 5), (OVER, 0, 0)), ((80, 80, 512, 8, 3, 5), (OK, 0, 80)), ((80, 7, 512, 8, 3, 5), (SHORT, 0, 0)),
             ((80, 7, 512, 4, 3, 5), (OK, 73, 7)), ((80, 3, 512, 4, 3, 5), (SHORT, 0, 0)), ((80, 8, 512, 8, 3, 5), (OK, 72, 0)),
             ((80, 4, 512, 4, 3, 5), (OK, 76, 0)), ((80, 0, 512, 8, 3, 5), (OK, 80, 0)), ((80, 40, 512, 8, 3, -1), (SEQ, 0, 0)),
             ((80, 40, 512, 8, 3, 2 ** 31), (SEQ, 0, 0)), ((80, 40, 512, 8, 3, INT32_MAX), (OK, 40, 40)), ((80, 40, 512, 8, 3, 0), (OK, 40, 40))]
    out = (C.c_int * 5)()
    for args, want in cases:
        host.emu_send_plan(*args, out)
        assert tuple(out[:3]) == want, (args, tuple(out))
        if want[0] == OK:
            assert out[3] == args[0] - args[1] and out[4] == args[5]


def _inputs(rng, n, P, slot):
    """random length records: valid packets, empties, every refusal reason, all four masks, sequence numbers around both int32 ends"""
    total = rng.integers(1, slot + 1, (n, P))
    n1 = np.where(rng.random((n, P)) < 0.1, 0, (rng.random((n, P)) * (total + 1)).astype(np.int64))
    kind = rng.random((n, P))
    total = np.where(kind < 0.10, rng.integers(-2, 1, (n, P)), total)                       # empty (n1 is then anything)
    total = np.where((kind >= 0.10) & (kind < 0.14), slot + rng.integers(1, 4, (n, P)), total)
    n1 = np.where((kind >= 0.14) & (kind < 0.18), -rng.integers(1, 4, (n, P)), n1)
    n1 = np.where((kind >= 0.18) & (kind < 0.22), total + rng.integers(1, 4, (n, P)), n1)
    n1 = np.where((kind >= 0.22) & (kind < 0.30), rng.integers(1, 10, (n, P)), n1)          # around both hbb values
    nbytes = np.stack([total, n1], axis=-1).astype(np.int16)
    send = rng.integers(0, 4, (n, P)).astype(np.uint8)
    seq_base = rng.integers(0, 1000, n).astype(np.int32)
    seq_base[::7] = INT32_MAX - rng.integers(0, P, seq_base[::7].size)                      # runs over the top inside the call
    seq_base[3::11] = -rng.integers(1, P, seq_base[3::11].size)                             # starts below zero
    return nbytes, send, seq_base


def _run_host(host, bits, nbytes, send, seq_base, first_seq, hbb, streams, max_records, cap, guard=64):
    n, P, slot = bits.shape
    FILL_R, FILL_P = -7, 0xA5
    rec = np.full((max_records + guard, 5), FILL_R, np.int32)
    pay = np.full(cap + guard + 3, FILL_P, np.uint8)
    pay_v = pay[3:]                                               # (a pool that starts at an odd address)
    cnt = np.zeros(8, np.int32)
    p = lambda x: x.ctypes.data if x is not None else None
    host.emu_send_pack(p(bits), p(nbytes), p(send), p(seq_base), p(streams), n, P, slot, hbb, first_seq, p(rec), max_records, p(pay_v), cap, p(cnt))
    c = dict(records=int(cnt[0]), records_needed=int(cnt[1]), bytes=int(cnt[2:4].view(np.int64)[0]), bytes_needed=int(cnt[4:6].view(np.int64)[0]),
             empty=int(cnt[6]), refused=int(cnt[7]))
    assert (rec[max_records:] == FILL_R).all() and (pay_v[cap:] == FILL_P).all() and (pay[:3] == FILL_P).all()
    assert (rec[c["records"]:] == FILL_R).all() and (pay_v[c["bytes"]:] == FILL_P).all()      # nothing behind what was written either
    return rec[:c["records"]], pay_v[:c["bytes"]], c


@pytest.mark.parametrize("hbb", [8, 4])
@pytest.mark.parametrize("slot,mapped", [(96, False), (97, True)])
def test_host_passes_against_model(host, hbb, slot, mapped):
    rng = np.random.default_rng(1000 + hbb + slot)
    n, P = 37, 23                                                 # 851 packets: four tiles, the last one partly filled
    backing = rng.integers(0, 256, n * P * slot + 5, dtype=np.uint8)
    bits = backing[1:1 + n * P * slot].reshape(n, P, slot)        # (slots at odd addresses, with slot = 97 at every alignment)
    nbytes, send, seq_base = _inputs(rng, n, P, slot)
    streams = np.sort(rng.choice(200, n, replace=False)).astype(np.int32) if mapped else None
    first_seq = 5
    full = model_pack(bits, nbytes, send, seq_base, first_seq, hbb, streams)
    assert all(full["reasons"][r] > 0 for r in REASONS), full["reasons"]
    assert full["count"]["empty"] > 0 and full["count"]["refused"] > 0
    assert set(np.unique(send)) == {0, 1, 2, 3}
    allr = full["all_records"]
    need_r, need_b = allr.shape[0], int(allr[:, 4].sum())
    assert need_r > 300
    # the caps: none; a record boundary between two packets; inside a packet, between its two datagrams (by count, and by bytes);
    # a byte short of a record's end; zero records; zero bytes
    ks = [k for k in range(50, need_r) if allr[k, 2] == 1 and allr[k - 1, 2] == 0 and (allr[k, :2] == allr[k - 1, :2]).all()]
    kb = [k for k in range(50, need_r) if allr[k, 2] == 0]
    k_in, k_edge = ks[len(ks) // 2], kb[len(kb) // 3]
    caps = [(need_r, need_b), (2 * n * P, n * P * slot), (k_edge, need_b), (k_in, need_b), (need_r, int(allr[k_in, 3])),
            (need_r, int(allr[k_in, 3] + allr[k_in, 4] - 1)), (need_r, int(allr[k_edge, 3])), (0, need_b), (need_r, 0), (0, 0), (k_in, int(allr[k_edge, 3]))]
    for max_records, cap in caps:
        want = model_pack(bits, nbytes, send, seq_base, first_seq, hbb, streams, max_records, cap)
        rec, pay, cnt = _run_host(host, bits, nbytes, send, seq_base, first_seq, hbb, streams, max_records, cap)
        assert cnt == want["count"], (max_records, cap, cnt, want["count"])
        assert np.array_equal(rec, want["records"]), (max_records, cap)
        assert np.array_equal(pay, want["payload"]), (max_records, cap)
        assert cnt["records_needed"] == need_r and cnt["bytes_needed"] == need_b
    # the cut inside a packet did cut between its two datagrams
    want = model_pack(bits, nbytes, send, seq_base, first_seq, hbb, streams, k_in, need_b)
    assert want["records"][-1, 2] == 0 and (allr[k_in, :2] == want["records"][-1, :2]).all()
    # no mask and no sequence base: everything of every valid packet
    want = model_pack(bits, nbytes, None, None, 0, hbb, streams)
    rec, pay, cnt = _run_host(host, bits, nbytes, None, None, 0, hbb, streams, 2 * n * P, n * P * slot)
    assert cnt == want["count"] and np.array_equal(rec, want["records"]) and np.array_equal(pay, want["payload"])


def test_copy_at_every_alignment(host):
    rng = np.random.default_rng(3)
    src = rng.integers(0, 256, 256, dtype=np.uint8)
    for da in range(4):
        for sa in range(4):
            for n in list(range(0, 24)) + [77, 78, 79, 80, 129]:
                dst = np.full(256, 0x5A, np.uint8)
                base_d = (-dst.ctypes.data) % 4 + 8 + da
                base_s = (-src.ctypes.data) % 4 + 8 + sa
                host.emu_send_copy(dst.ctypes.data + base_d, src.ctypes.data + base_s, n)
                assert np.array_equal(dst[base_d:base_d + n], src[base_s:base_s + n]), (da, sa, n)
                assert (dst[:base_d] == 0x5A).all() and (dst[base_d + n:] == 0x5A).all(), (da, sa, n)


def test_wave_scan_host_form_against_cumsum(host):
    rng = np.random.default_rng(4)
    for it in range(200):
        if it % 3 == 0:
            v = rng.integers(-2 ** 31, 2 ** 31, 64).astype(np.int32)        # the sums wrap
        elif it % 3 == 1:
            v = rng.integers(0, 600, 64).astype(np.int32)
        else:
            v = np.zeros(64, np.int32); v[int(rng.integers(0, 32))] = INT32_MAX; v[int(rng.integers(32, 64))] = 1
        want = (np.cumsum(v.astype(np.int64)) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
        got = v.copy()
        host.emu_wave_scan(got.ctypes.data)
        assert np.array_equal(got, want), it


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="no LLVM binutils on this box")
def test_send_kernels_use_no_scratch():
    import solo_amd
    if not os.path.exists(solo_amd.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    sys.path.insert(0, os.path.join(T.ROOT, "tools"))
    from kernel_resources import kernel_resources
    seen = kernel_resources(solo_amd.LIB_PATH)
    for frag in ("solo_send_totals_kernel", "solo_send_scan_kernel", "solo_send_scatter_kernel"):
        hits = [r for name, r in seen.items() if frag in name]
        assert len(hits) == 1, (frag, len(hits))                  # rate-independent: compiled once
        assert hits[0]["scratch"] == 0, (frag, hits[0])

"""solo_rate (include/solo_mi355x.h): the symbols exist, the Python layer knows them, the records have one layout in the header, in ctypes
and in the host build, and every host refusal the header lists for solo_batch_update_rates, solo_rate_update and solo_rate_send_mask
returns "refused" from the very checks the entry points run (solo_amd/csrc/solo_rate.h, through the host build of tests/rate_host.cpp: no
GPU call is made here)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import rate_model as M
import solo_amd
import solo_testlib as T
from host_build import host_lib

SYMBOLS = ("solo_batch_update_rates", "solo_rate_create", "solo_rate_destroy", "solo_rate_reset", "solo_rate_reset_rows", "solo_rate_get_state",
           "solo_rate_set_state", "solo_rate_update", "solo_rate_send_mask")


@pytest.fixture(scope="module")
def host():
    lib = host_lib("rate")
    lib.emu_rate_init.argtypes = [C.c_void_p, C.c_int]
    lib.emu_rate_update_call_ok.argtypes = [C.c_int] + [C.c_void_p] * 5
    lib.emu_rate_apply_call_ok.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.emu_rate_mask_call_ok.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    return lib


def _header_fields(hdr, name):
    body = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % name, hdr).group(1)
    return [f.strip() for f in re.sub(r"\b(u?int32_t)\b", "", body).replace(";", ",").split(",") if f.strip()]


def test_symbols_and_layouts(host):
    if not os.path.exists(solo_amd.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = C.CDLL(solo_amd.LIB_PATH)
    for s in SYMBOLS:
        assert s in solo_amd.ABI_SYMBOLS and hasattr(lib, s), s
    hdr = open(os.path.join(T.ROOT, "include", "solo_mi355x.h")).read()
    assert "#define SOLO_RATE_STATE_BYTES 64" in hdr
    assert solo_amd.RATE_STATE_BYTES == host.emu_rate_state_bytes() == M.STATE_BYTES == 64 and solo_amd.Rate.state_bytes == 64
    for struct, size, host_size, names in ((solo_amd.solo_rate_apply_count_t, 16, host.emu_rate_apply_count_size(), M.APPLY_COUNT),
                                           (solo_amd.solo_rate_params_t, 48, host.emu_rate_params_size(), M.PARAMS),
                                           (solo_amd.solo_rate_count_t, 64, host.emu_rate_count_size(), M.COUNT + ("reserved0", "reserved1"))):
        assert C.sizeof(struct) == size == host_size, struct
        assert tuple(n for n, _ in struct._fields_) == tuple(names), struct
        want = [n for n in names if not re.fullmatch(r"reserved\d", n)] + (["reserved[2]"] if struct is solo_amd.solo_rate_count_t else [])
        assert _header_fields(hdr, struct.__name__) == want, struct
    assert C.sizeof(solo_amd.solo_rtcp_feedback_t) == host.emu_rate_feedback_size() == 32
    assert solo_amd.Rate.COUNT == M.COUNT and solo_amd.SoloBatch.RATES_COUNT == M.APPLY_COUNT
    st = np.full((3, 16), 0x5A5A5A5A, dtype=np.int32)
    host.emu_rate_init(st.ctypes.data, 3)
    assert np.array_equal(st, np.tile(np.array(M.INIT, dtype=np.int64).astype(np.int32), (3, 1))) and M.INIT[3] == 2 ** 31 - 1 and sum(M.INIT) == M.INIT[3]
    sig = inspect.signature(solo_amd.Rate.update)
    assert {k: v.default for k, v in sig.parameters.items() if k in M.DEFAULTS} == M.DEFAULTS
    assert issubclass(solo_amd.Rate, solo_amd._RowStateObject) and hasattr(solo_amd.SoloBatch, "update_rates") and hasattr(solo_amd.Rate, "send_mask")


@pytest.fixture()
def addr():
    buf = np.zeros(64, dtype=np.int32)
    a = (buf.ctypes.data + 63) & ~63                        # (never dereferenced: the checks look at addresses only)
    yield a
    del buf


def test_update_rates_refusals(host, addr):
    lst, tgt, cnt = addr, addr + (1 << 20), addr + (1 << 21)

    def ok(N=8, enc=1, streams=lst, n=3, target=tgt, count=cnt):
        return host.emu_rate_apply_call_ok(N, enc, streams, n, target, count)
    assert ok() == 1 and ok(streams=None, n=8) == 1 and ok(n=8) == 1 and ok(n=1) == 1
    assert ok(target=None) == 0 and ok(count=None) == 0
    assert ok(enc=0) == 0                                   # the handle has no encoder
    for n in (0, -1, 9, 2 ** 31 - 1):
        assert ok(n=n) == 0, n
    for n in (1, 3, 7, 9):
        assert ok(streams=None, n=n) == 0, n                # without a list n must be N
    for off in (1, 2, 3):
        assert ok(streams=lst + off) == 0 and ok(target=tgt + off) == 0 and ok(count=cnt + off) == 0, off
    assert ok(streams=lst + 4, target=tgt + 4, count=cnt + 4) == 1


def test_rate_update_refusals(host, addr):
    fb, tgt, mode, cnt = addr, addr + (1 << 20), addr + (1 << 21), addr + (1 << 22)
    good = M.params_words(M.params(6000, 40000, 16000))

    def ok(n_rows=8, feedback=fb, p=good, target=tgt, mode=mode, count=cnt):
        return host.emu_rate_update_call_ok(n_rows, feedback, None if p is None else p.ctypes.data, target, mode, count)
    assert ok() == 1 and ok(mode=mode + 1) == 1 and ok(n_rows=1 << 24) == 1
    assert ok(feedback=None) == 0 and ok(p=None) == 0 and ok(target=None) == 0 and ok(mode=None) == 0 and ok(count=None) == 0
    assert ok(n_rows=0) == 0 and ok(n_rows=-1) == 0
    for off in (4, 8, 12, 1):
        assert ok(feedback=fb + off) == 0, off
    for off in (1, 2, 3):
        assert ok(target=tgt + off) == 0 and ok(count=cnt + off) == 0, off
    assert ok(target=tgt + 4, count=cnt + 4, feedback=fb + 16) == 1
    for kw in (dict(min_bps=40200), dict(start_bps=5800), dict(quantum_bps=0), dict(min_bps=6100), dict(max_bps=1000200), dict(lo_q8=27), dict(hi_q8=256),
               dict(inc_q8=257), dict(rtt_guard=-1), dict(stale_calls=-1), dict(thin_after=-1), dict(thin_release=-1), dict(reserved=1)):
        assert ok(p=M.params_words(dict(M.params(6000, 40000, 16000), **kw))) == 0, kw


def test_send_mask_refusals(host, addr):
    mode, lst, base, send = addr, addr + (1 << 20), addr + (1 << 21), addr + (1 << 22)

    def ok(mode=mode, n_rows=8, streams=None, n=8, P=2, seq_base=None, send=send):
        return host.emu_rate_mask_call_ok(mode, n_rows, streams, n, P, seq_base, send)
    assert ok() == 1 and ok(streams=lst, n=3, seq_base=base) == 1 and ok(n=3) == 1 and ok(mode=mode + 1, send=send + 3) == 1
    assert ok(mode=None) == 0 and ok(send=None) == 0
    for v in (0, -1):
        assert ok(n=v) == 0 and ok(P=v) == 0 and ok(n_rows=v, n=1) == 0, v
    assert ok(n=9) == 0 and ok(streams=lst, n=9) == 0
    big = 1 << 20
    assert ok(n_rows=big, n=big, P=2048) == 0 and ok(n_rows=big, n=big, P=2047) == 1       # n * n_packets below 2^31
    assert ok(n_rows=1, n=1, P=2 ** 31 - 1) == 1
    for off in (1, 2, 3):
        assert ok(seq_base=base + off) == 0 and ok(streams=lst + off, n=3) == 0, off
    assert ok(seq_base=base + 4, streams=lst + 4, n=3) == 1

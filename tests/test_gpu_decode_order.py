"""Decode calls of one handle issued on different streams without a host synchronisation: the library orders a decode call behind the
one before it, and a reset behind the latest decode call, whichever streams they were issued on; the calls share the stream states, the
buffer of extraction records and the subset verdict word.  Every case runs as one chunk per call (the default) and with
SOLO_DEC_CHUNK=3, SOLO_DEC_FIRST_CHUNK=2, where a call of 7 packets is cut 2 + 3 + 2 and every chunk reuses the one buffer.
Expected PCM: the reference decoder's, stored in tests/golden/synth8x25.npz (8 streams x 25 packets, with description loss)."""
import os

import numpy as np
import pytest

import solo_testlib as T

pytestmark = pytest.mark.gpu

KNOBS = [{}, {"SOLO_DEC_CHUNK": "3", "SOLO_DEC_FIRST_CHUNK": "2"}]
CUT = 7                                    # call A decodes packets 0 .. CUT - 1
SLEEP_TICKS = 5_000_000                    # ~50 ms of the device's 100 MHz counter: call A is still pending when the next call is issued


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(T.GOLDEN, "synth8x25.npz"))
    return {k: z[k] for k in ("bits", "nbytes", "recv", "dec_loss")}


class _Case:
    """a fresh decoder handle under `knobs`, the fixture's inputs on the device cut into packet ranges, and the outputs of every call
    allocated ahead of the calls: nothing but the library orders the calls"""

    def __init__(self, torch, monkeypatch, golden, knobs):
        import solo_amd
        for k, v in knobs.items():
            monkeypatch.setenv(k, v)                                        # read at the handle's first decode
        self.torch, self.g = torch, golden
        self.N, self.P, S = golden["bits"].shape
        self.b = solo_amd.SoloBatch(self.N, encoder=False, decoder=True, slot_bytes=S)

    def inputs(self, p0, p1, rows=None):
        """(bits, nbytes, recv, pcm, status) of a call over packets p0 .. p1 - 1 of `rows` (None: every stream); the status starts non-zero"""
        rows = list(range(self.N)) if rows is None else rows
        dev = lambda a: self.torch.from_numpy(np.ascontiguousarray(a[rows, p0:p1])).to("cuda")
        out = self.torch.zeros((len(rows), p1 - p0, 640), dtype=self.torch.int16, device="cuda")
        st = self.torch.full((len(rows),), 77, dtype=self.torch.int32, device="cuda")
        return dev(self.g["bits"]), dev(self.g["nbytes"]), dev(self.g["recv"]), out, st

    def decode(self, stream, a, delay=False, **kw):
        bits, nb, rv, out, st = a
        with self.torch.cuda.stream(stream):
            if delay:
                self.torch.cuda._sleep(SLEEP_TICKS)
            self.b.decode(bits, nb, rv, pcm=out, status=st, **kw)
        return out, st


def _host(*tensors):
    return [t.cpu().numpy() for t in tensors]


@pytest.mark.parametrize("knobs", KNOBS, ids=["one_chunk", "chunks_2_3"])
def test_two_streams_no_host_sync(torch_cuda, monkeypatch, golden, knobs):
    """call A (packets 0..6) on a delayed stream, call B (7..24) on another: B continues A's states and reuses A's record buffer"""
    torch = torch_cuda
    c = _Case(torch, monkeypatch, golden, knobs)
    a, b = c.inputs(0, CUT), c.inputs(CUT, c.P)
    torch.cuda.synchronize()
    X, Y = torch.cuda.Stream(), torch.cuda.Stream()
    outA, stA = c.decode(X, a, delay=True)
    outB, stB = c.decode(Y, b)
    torch.cuda.synchronize()
    outA, stA, outB, stB = _host(outA, stA, outB, stB)
    assert not stA.any() and not stB.any()
    assert np.array_equal(np.concatenate([outA, outB], axis=1), golden["dec_loss"])


@pytest.mark.parametrize("knobs", KNOBS, ids=["one_chunk", "chunks_2_3"])
def test_reset_behind_decode_on_another_stream(torch_cuda, monkeypatch, golden, knobs):
    """a reset on Y waits for the decode still pending on X: the full decode after it starts from fresh states"""
    torch = torch_cuda
    c = _Case(torch, monkeypatch, golden, knobs)
    a, full = c.inputs(0, CUT), c.inputs(0, c.P)
    torch.cuda.synchronize()
    X, Y = torch.cuda.Stream(), torch.cuda.Stream()
    c.decode(X, a, delay=True)
    with torch.cuda.stream(Y):
        c.b.reset()
    out, st = c.decode(Y, full)
    torch.cuda.synchronize()
    out, st = _host(out, st)
    assert not st.any()
    assert np.array_equal(out, golden["dec_loss"])


@pytest.mark.parametrize("knobs", KNOBS, ids=["one_chunk", "chunks_2_3"])
def test_buffer_growth_between_calls(torch_cuda, monkeypatch, golden, knobs):
    """the second call (23 packets after 2) needs a larger record buffer than the first left (also with chunks of 3: the first call's
    buffer holds 2 packets); the third call, after a reset, fits what is there"""
    torch = torch_cuda
    c = _Case(torch, monkeypatch, golden, knobs)
    a, b, full = c.inputs(0, 2), c.inputs(2, c.P), c.inputs(0, c.P)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    outA, stA = c.decode(s, a)
    outB, stB = c.decode(s, b)
    with torch.cuda.stream(s):
        c.b.reset()
    outF, stF = c.decode(s, full)
    torch.cuda.synchronize()
    outA, stA, outB, stB, outF, stF = _host(outA, stA, outB, stB, outF, stF)
    assert not stA.any() and not stB.any() and not stF.any()
    assert np.array_equal(np.concatenate([outA, outB], axis=1), golden["dec_loss"])
    assert np.array_equal(outF, golden["dec_loss"])


@pytest.mark.parametrize("knobs", KNOBS, ids=["one_chunk", "chunks_2_3"])
def test_subset_call_behind_full_call(torch_cuda, monkeypatch, golden, knobs):
    """a subset call on Y behind a full decode of packets 0..6 pending on X: it shares that call's record buffer, and the verdict word
    of its list is written behind it.  Streams 2, 5, 7: a list must be strictly increasing."""
    torch = torch_cuda
    c = _Case(torch, monkeypatch, golden, knobs)
    rows = [2, 5, 7]
    a, sub = c.inputs(0, CUT), c.inputs(CUT, 2 * CUT, rows)
    torch.cuda.synchronize()
    X, Y = torch.cuda.Stream(), torch.cuda.Stream()
    c.decode(X, a, delay=True)
    out, st = c.decode(Y, sub, streams=rows)
    torch.cuda.synchronize()
    out, st = _host(out, st)
    assert not st.any()
    assert np.array_equal(out, golden["dec_loss"][rows, CUT:2 * CUT])

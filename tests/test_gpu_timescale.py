"""Play-out time scaling on the GPU (solo_timescale through the binding and the raw C ABI): every output sample, shift, cost and the count
against the independent numpy model of tests/timescale_model.py (67 rows of every input family, seven packet ratios, the four packet
geometries), the refusals, and the whole path -- the reference encoder's packets -> ring -> play-out of two packets (or of one with a
description lost) -> time scaling -- against the compiled reference decoder followed by the same model."""
import numpy as np
import pytest

import refcodec as R
from timescale_model import FAMILIES, GEOMETRIES, geometry, model_timescale, timescale_rows

need_ref = pytest.mark.skipif(not R.have_ref("fix"), reason="oracle/_ref not present")
pytestmark = pytest.mark.gpu
FILL_O, FILL_S, FILL_C, FILL_N = 0x1234, -77, -99, 0x5A5A5A5A
GUARD = 3
N = 67
RATIOS = ((1, 1), (2, 1), (3, 2), (1, 2), (2, 3), (4, 1), (1, 4))


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch


def _handle(fs, L, n=4, **kw):
    import solo_amd
    kw.setdefault("encoder", False)
    h = solo_amd.SoloBatch(n, samplerate=fs, framesize_ms=40 * L * 16000 // (640 * fs), **kw)
    assert h.packet_samples == L and h.samplerate == fs
    return h


def _scale_and_compare(torch, h, pcm, b, raw):
    """solo_timescale into pre-filled buffers with guard rows, through the binding or the C ABI (raw); everything against the model"""
    n, a, L = pcm.shape
    M = geometry(h.samplerate, L, a, b)["M"]
    d_pcm = torch.from_numpy(pcm).cuda()
    out = torch.full((n + GUARD, b, L), FILL_O, dtype=torch.int16, device="cuda")
    shift = torch.full((n + GUARD, M), FILL_S, dtype=torch.int32, device="cuda")
    cost = torch.full((n + GUARD, M), FILL_C, dtype=torch.int32, device="cuda")
    if raw:
        cnt = torch.full((4,), FILL_N, dtype=torch.int32, device="cuda")
        assert h.lib.solo_timescale(h.h, d_pcm.data_ptr(), n, a, b, out.data_ptr(), shift.data_ptr(), cost.data_ptr(), cnt.data_ptr(), h._stream()) == 0
    else:
        o, cnt = h.timescale(d_pcm, b, out=out[:n], shift=shift[:n], cost=cost[:n])
        assert o.data_ptr() == out.data_ptr()
    c = h.timescale_count(cnt)
    want = model_timescale(pcm, b, h.samplerate)
    assert c == want["count"], (a, b, c, want["count"])
    ho, hs, hc = out.cpu().numpy(), shift.cpu().numpy(), cost.cpu().numpy()
    bad = np.argwhere((ho[:n] != want["out"]).any(axis=2))
    assert len(bad) == 0, (a, b, bad[:8].tolist())
    assert np.array_equal(hs[:n], want["shift"]) and np.array_equal(hc[:n], want["cost"]), (a, b)
    assert (ho[n:] == FILL_O).all() and (hs[n:] == FILL_S).all() and (hc[n:] == FILL_C).all()          # the guard rows keep their fill
    assert np.array_equal(d_pcm.cpu().numpy(), pcm)
    return want


@pytest.mark.parametrize("fs,L", GEOMETRIES)
def test_gpu_model_parity(torch_cuda, fs, L):
    """67 rows (one wavefront each) of speech, full-scale noise, +-full-scale squares, constants, impulses and periodic rows"""
    h = _handle(fs, L)
    by_abs = by_sign = 0
    for k, (a, b) in enumerate(RATIOS):
        pcm, fam = timescale_rows(300 * a + b, N, fs, L, a, b)
        assert all((fam == f).sum() >= N // 6 for f in range(len(FAMILIES)))
        want = _scale_and_compare(torch_cuda, h, pcm, b, raw=k % 2 == 1)
        by_abs, by_sign = by_abs + int(want["by_abs"].sum()), by_sign + int(want["by_sign"].sum())
        if a == b:
            assert np.array_equal(want["out"], pcm)
        if (a, b) == (4, 1):
            assert want["cost"].max() == 2 * (fs // 200) * 65535                       # the bound of a cost is reached
    assert by_abs > 0 and by_sign > 0                                                  # ties were decided both ways
    h.close()


def test_gpu_without_side_outputs_or_count(torch_cuda):
    torch = torch_cuda
    fs, L, a, b, n = 16000, 640, 3, 2, 9
    h = _handle(fs, L)
    pcm, _ = timescale_rows(5, n, fs, L, a, b)
    want = model_timescale(pcm, b, fs)
    out = torch.full((n + GUARD, b, L), FILL_O, dtype=torch.int16, device="cuda")
    assert h.lib.solo_timescale(h.h, torch.from_numpy(pcm).cuda().data_ptr(), n, a, b, out.data_ptr(), None, None, None, h._stream()) == 0
    ho = out.cpu().numpy()
    assert np.array_equal(ho[:n], want["out"]) and (ho[n:] == FILL_O).all()
    h.close()


def test_gpu_refusals(torch_cuda):
    torch = torch_cuda
    fs, L, n = 16000, 640, 4
    h = _handle(fs, L)
    x = torch.zeros((n + 1, 2, L), dtype=torch.int16, device="cuda")
    out = torch.full((n, 4, L), FILL_O, dtype=torch.int16, device="cuda")
    side = torch.full((n, 32), FILL_S, dtype=torch.int32, device="cuda")
    cnt = torch.full((4,), FILL_N, dtype=torch.int32, device="cuda")

    def call(handle=h.h, pin=x.data_ptr(), n=n, a=2, b=1, pout=out.data_ptr()):
        return h.lib.solo_timescale(handle, pin, n, a, b, pout, side.data_ptr(), side.data_ptr(), cnt.data_ptr(), h._stream())

    assert call(handle=None) == -1 and call(pin=None) == -1 and call(pout=None) == -1 and call(n=0) == -1 and call(n=-1) == -1
    assert call(a=0) == -1 and call(a=5) == -1 and call(b=0) == -1 and call(b=5) == -1
    assert call(n=-(-2 ** 31 // (2 * L))) == -1 and call(n=-(-2 ** 31 // (4 * L)), b=4) == -1              # n x max(a, b) x L reaches 2^31
    assert call(pin=x.data_ptr() + 2) == -1 and call(pout=out.data_ptr() + 8) == -1                        # not 16-byte aligned
    assert call(pout=x.data_ptr()) == -1                                                                   # in place
    assert call(pout=x.data_ptr() + (n * 2 - 1) * L * 2) == -1 and call(pin=out.data_ptr() + (n - 1) * L * 2) == -1     # overlapping by a packet
    torch.cuda.synchronize()
    assert bool((out == FILL_O).all()) and bool((side == FILL_S).all()) and bool((cnt == FILL_N).all())
    assert call() == 0                                                                                     # and the handle scales on afterwards
    flat = out.view(-1)                                                                                    # (the call's rows are [n][1][L])
    assert h.timescale_count(cnt) == dict(rows=n, blocks=n * 6, cost=0) and bool((flat[:n * L] == 0).all()) and bool((flat[n * L:] == FILL_O).all())
    h.close()


def test_gpu_binding_on_a_side_stream(torch_cuda):
    """through the binding, on a non-default stream, with out= given"""
    torch = torch_cuda
    fs, L, a, b, n = 32000, 1280, 2, 3, 21
    h = _handle(fs, L)
    pcm, _ = timescale_rows(11, n, fs, L, a, b)
    want = model_timescale(pcm, b, fs)
    d_pcm = torch.from_numpy(pcm).cuda()
    out = torch.full((n, b, L), FILL_O, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        o, cnt = h.timescale(d_pcm, b, out=out)
        plain, cnt2 = h.timescale(d_pcm, b)
    s.synchronize()
    assert o is out and np.array_equal(out.cpu().numpy(), want["out"]) and np.array_equal(plain.cpu().numpy(), want["out"])
    assert h.timescale_count(cnt) == want["count"] == h.timescale_count(cnt2)
    h.close()


@need_ref
def test_gpu_play_out_against_the_compiled_reference(torch_cuda):
    """8 streams at 13.6 kbps: the reference encoder's packets go into the ring; two packets are played and scaled 2 -> 1, then one packet
    with a description lost is played and scaled 1 -> 2; both equal the model applied to the reference decoder's PCM, byte for byte"""
    import solo_amd
    torch = torch_cuda
    NS, P, FIRST, L = 8, 5, 40, 640
    x = np.stack([R.synth_stream(900 + i, P) for i in range(NS)])
    arr, pool, ref = [], b"", np.zeros((NS, P, L), np.int16)
    for i in range(NS):
        e, d = R.RefEncoder("fix", rate=13600), R.RefDecoder("fix", use_md_index=0)
        for p in range(P):
            pl, n0, n1 = e.encode(x[i, p])
            keep = (True, True) if p < P - 1 else (i % 2 == 0, i % 2 == 1)             # the last packet loses one description
            for desc, (part, kept) in enumerate(zip((pl[:n0 - n1], pl[n0 - n1:n0]), keep)):
                if kept:
                    arr.append((i, FIRST + p, desc, len(pool), len(part)))
                    pool += part
            ref[i, p], ret = d.decode(*R.map_loss(pl, n0, n1, not keep[0], not keep[1]))
            assert ret == 0
    rx = solo_amd.SoloBatch(NS, encoder=False, decoder=True)
    rx.recv_create(8, 256, 0)
    rx.recv_reset_streams(list(range(NS)), FIRST)
    rx.recv_insert(torch.tensor(arr, dtype=torch.int32).cuda(), torch.from_numpy(np.frombuffer(pool, np.uint8).copy()).cuda())
    assert rx.recv_stats() == dict(inserted=len(arr), late=0, ahead=0, duplicate=0, bad=0)
    streams = list(range(NS))
    for tick in range(2):                                                              # packets 0 .. 3: two a tick, played at double speed
        two, st = rx.recv_decode(2, streams=streams)
        one, cnt = rx.timescale(two, 1)
        torch.cuda.synchronize()
        assert int(st.abs().max()) == 0 and np.array_equal(two.cpu().numpy(), ref[:, 2 * tick:2 * tick + 2])
        want = model_timescale(ref[:, 2 * tick:2 * tick + 2], 1, 16000)
        assert np.array_equal(one.cpu().numpy(), want["out"]) and rx.timescale_count(cnt) == want["count"]
    assert want["count"]["cost"] > 0 and not np.array_equal(want["out"][:, 0], ref[:, 2]) and np.abs(ref[:, 2:4].astype(np.int32)).mean() > 100
    last, st = rx.recv_decode(1, streams=streams)                                      # packet 4, half of it lost: stretched to two
    two, cnt = rx.timescale(last, 2)
    torch.cuda.synchronize()
    assert int(st.abs().max()) == 0 and np.array_equal(last.cpu().numpy(), ref[:, 4:5])
    want = model_timescale(ref[:, 4:5], 2, 16000)
    assert np.array_equal(two.cpu().numpy(), want["out"]) and rx.timescale_count(cnt) == want["count"] and want["count"]["cost"] > 0
    rx.close()

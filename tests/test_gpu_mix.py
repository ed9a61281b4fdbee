"""Mixing bridge on the GPU (solo_mix through the binding and the raw C ABI): every output sample, the energies, the flags and the count
against the independent numpy model of tests/mix_model.py (the small case with everything the interface names, 4096 x 50, 2048 x 10 at
32 kHz, 20 ms packets), the refusals, the unity check, and the whole bridge -- encode -> pack -> ring -> play-out -> mix -> encode --
against the compiled reference codec around the same model."""
import ctypes as C

import numpy as np
import pytest

import refcodec as R
from mix_model import GAINS, mix_case, model_mix, ties_decide

need_ref = pytest.mark.skipif(not R.have_ref("fix"), reason="oracle/_ref not present")
pytestmark = pytest.mark.gpu
FILL_O, FILL_E, FILL_M, FILL_C = 0x1234, -77, 0xA5, 0x5A5A5A5A
GUARD = 3
FRONT_END_BYTES = 252            # what the receiver front end takes per packet (tests/test_gpu_rate_range.py pins it)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch


def _handle(L, n=4, **kw):
    import solo_amd
    samplerate, framesize_ms = {640: (16000, 40), 1280: (32000, 40), 320: (16000, 20)}[L]
    kw.setdefault("encoder", False)
    h = solo_amd.SoloBatch(n, samplerate=samplerate, framesize_ms=framesize_ms, **kw)
    assert h.packet_samples == L
    return h


def _buffers(torch, n, P, L):
    out = torch.full((n + GUARD, P, L), FILL_O, dtype=torch.int16, device="cuda")
    energy = torch.full((n + GUARD, P), FILL_E, dtype=torch.int64, device="cuda")
    mixed = torch.full((n + GUARD, P), FILL_M, dtype=torch.uint8, device="cuda")
    return out, energy, mixed


def _untouched(out, energy, mixed):
    return bool((out == FILL_O).all()) and bool((energy == FILL_E).all()) and bool((mixed == FILL_M).all())


def _mix_and_compare(torch, h, pcm, room, gain, max_speakers, raw_n_rooms=None):
    """solo_mix into pre-filled buffers with guard rows, through the binding (raw_n_rooms None) or the C ABI; everything against the model"""
    n, P, L = pcm.shape
    d_pcm, d_room = torch.from_numpy(pcm).cuda(), torch.from_numpy(room).cuda()
    d_gain = None if gain is None else torch.from_numpy(gain).cuda()
    out, energy, mixed = _buffers(torch, n, P, L)
    if raw_n_rooms is None:
        o, cnt = h.mix(d_pcm, d_room, gain=d_gain, max_speakers=max_speakers, out=out[:n], energy=energy[:n], mixed=mixed[:n])
        assert o.data_ptr() == out.data_ptr()
        n_rooms = n
    else:
        cnt = torch.full((4,), FILL_C, dtype=torch.int32, device="cuda")
        ret = h.lib.solo_mix(h.h, d_pcm.data_ptr(), n, P, d_room.data_ptr(), raw_n_rooms, None if gain is None else d_gain.data_ptr(), max_speakers,
                             out.data_ptr(), energy.data_ptr(), mixed.data_ptr(), cnt.data_ptr(), h._stream())
        assert ret == 0
        n_rooms = raw_n_rooms
    c = h.mix_count(cnt)
    pad = lambda a: np.concatenate([a, np.zeros((GUARD,) + a.shape[1:], a.dtype)])
    want = model_mix(pad(pcm), np.concatenate([room, np.full(GUARD, -1, np.int32)]), n_rooms, None if gain is None else pad(gain), max_speakers,
                     out=np.full((n + GUARD, P, L), FILL_O, np.int16), energy=np.full((n + GUARD, P), FILL_E, np.int64),
                     mixed=np.full((n + GUARD, P), FILL_M, np.uint8))
    print("solo_mix %d x %d x %d, max_speakers %d: count %s" % (n, P, L, max_speakers, c))
    assert c == want["count"], (c, want["count"])
    ho = out.cpu().numpy()
    bad = np.argwhere((ho != want["out"]).any(axis=2))
    assert len(bad) == 0, bad[:8].tolist()
    assert np.array_equal(energy.cpu().numpy(), want["energy"]) and np.array_equal(mixed.cpu().numpy(), want["mixed"])
    assert (ho[n:] == FILL_O).all() and (ho[:n][room < 0] == FILL_O).all()          # guards and rows in no room keep their fill
    return want


@pytest.mark.parametrize("L", [640, 1280, 320])
def test_gpu_model_parity_small(torch_cuda, L):
    """rooms of 1, 2, 3, 64, 65 and 1000, rows in no room, every gain, full-scale rows, tied energies; max_speakers 0, 1, 3, 64"""
    P = 3
    pcm, room, gain, n_rooms = mix_case(200 + L, P, L)
    sizes = set(np.bincount(room[room >= 0]).tolist())
    assert {1, 2, 3, 64, 65, 1000} <= sizes and (room == -1).sum() >= 10 and set(GAINS) <= set(gain.tolist())
    h = _handle(L)
    for k, max_speakers in enumerate([0, 1, 3, 64]):
        want = _mix_and_compare(torch_cuda, h, pcm, room, gain, max_speakers, raw_n_rooms=n_rooms if k % 2 else None)
        assert want["count"]["clipped"] > 0
        if max_speakers:
            assert ties_decide(want["energy"][:len(room)], room, max_speakers) > 0
    _mix_and_compare(torch_cuda, h, pcm, room, None, 3, raw_n_rooms=n_rooms)      # NULL gain
    _mix_and_compare(torch_cuda, h, pcm, room, None, 0)
    h.close()


def _floor(seed, n, sizes):
    """n rows in rooms whose sizes cycle through `sizes`, scattered; the last few rows in no room"""
    rng = np.random.default_rng(seed)
    room = np.full(n, -1, np.int32)
    rows, k, r = rng.permutation(n), 0, 0
    while k + sizes[r % len(sizes)] <= n - 5:
        m = sizes[r % len(sizes)]
        room[rows[k:k + m]] = r
        k, r = k + m, r + 1
    return room, rng


@pytest.mark.parametrize("n,P,L,sizes", [(4096, 50, 640, (2, 8, 3, 2, 5, 200)), (2048, 10, 1280, (2, 6, 9, 70))])
def test_gpu_model_parity_large(torch_cuda, n, P, L, sizes):
    room, rng = _floor(n + P, n, sizes)
    level = rng.integers(0, 10, (n, P, 1))
    pcm = (rng.integers(-32768, 32768, (n, P, L), dtype=np.int16) >> level).astype(np.int16)
    gain = rng.integers(-100, 8192, n).astype(np.int16)
    h = _handle(L)
    want = _mix_and_compare(torch_cuda, h, pcm, room, gain, 3)
    assert want["count"]["rows"] >= n - 300 and want["count"]["clipped"] > 0
    _mix_and_compare(torch_cuda, h, pcm, room, gain, 0, raw_n_rooms=int(room.max()) + 1)
    h.close()


def test_gpu_unity(torch_cuda):
    """2-member rooms, NULL gain, every member mixed: each row's output is the other row's input, exactly"""
    torch = torch_cuda
    rng = np.random.default_rng(5)
    n, P, L = 512, 6, 640
    pcm = rng.integers(-32768, 32768, (n, P, L), dtype=np.int16)
    room = (rng.permutation(n) // 2).astype(np.int32)
    other = np.empty(n, np.int64)
    for r in range(n // 2):
        a, b = np.flatnonzero(room == r)
        other[a], other[b] = b, a
    h = _handle(L)
    out, cnt = h.mix(torch.from_numpy(pcm).cuda(), torch.from_numpy(room).cuda())
    assert h.mix_count(cnt) == dict(rows=n, rooms=n // 2, clipped=0)
    assert np.array_equal(out.cpu().numpy(), pcm[other])
    h.close()


def test_gpu_refusals(torch_cuda):
    torch = torch_cuda
    n, P, L = 16, 2, 640
    h = _handle(L)
    lib = h.lib
    pcm = torch.zeros((n + 1, P, L), dtype=torch.int16, device="cuda")
    room = torch.zeros((8192,), dtype=torch.int32, device="cuda")
    out, energy, mixed = _buffers(torch, n, P, L)
    cnt = torch.full((4,), FILL_C, dtype=torch.int32, device="cuda")
    big_in = torch.zeros((8192, 1, L), dtype=torch.int16, device="cuda")
    big_out = torch.full((8192, 1, L), FILL_O, dtype=torch.int16, device="cuda")

    def call(handle=h.h, pin=pcm.data_ptr(), n=n, P=P, room=room.data_ptr(), n_rooms=4, K=0, pout=out.data_ptr()):
        return lib.solo_mix(handle, pin, n, P, room, n_rooms, None, K, pout, energy.data_ptr(), mixed.data_ptr(), cnt.data_ptr(), h._stream())

    assert call(handle=None) == -1 and call(pin=None) == -1 and call(room=None) == -1 and call(pout=None) == -1
    assert call(n=0) == -1 and call(n=-3) == -1 and call(P=0) == -1 and call(n_rooms=0) == -1 and call(n_rooms=n + 1) == -1
    assert call(n=2, P=2 ** 30, n_rooms=1) == -1                                       # n * n_packets = 2^31
    assert call(K=65) == -1
    assert call(pin=big_in.data_ptr(), pout=big_out.data_ptr(), n=8192, P=1, K=0) == -1 and call(pin=big_in.data_ptr(), pout=big_out.data_ptr(), n=8192, P=1, K=-1) == -1
    assert call(pin=pcm.data_ptr() + 2) == -1 and call(pout=out.data_ptr() + 8) == -1    # not 16-byte aligned
    assert call(pout=pcm.data_ptr()) == -1                                             # in place
    assert call(pout=pcm.data_ptr() + P * L * 2) == -1 and call(pin=out.data_ptr() + (n - 1) * P * L * 2) == -1     # overlapping by a row
    torch.cuda.synchronize()
    assert _untouched(out, energy, mixed) and bool((cnt == FILL_C).all()) and bool((big_out == FILL_O).all())
    # a room id outside [-1, n_rooms): found on the device, rows = -1 and nothing else
    for bad in (4, -2, 2 ** 31 - 1):
        room[:n] = 0
        room[7] = bad
        assert call() == 0
        torch.cuda.synchronize()
        hc = cnt.cpu().numpy()
        assert hc[0] == -1 and (hc[1:] == FILL_C).all() and _untouched(out, energy, mixed), bad
        assert h.mix_count(cnt)["rows"] == -1
    # the binding takes n rooms: id n is refused, and the handle mixes on afterwards
    room[7] = n
    o, c2 = h.mix(pcm[:n], room[:n].contiguous(), out=out[:n])
    assert h.mix_count(c2)["rows"] == -1 and _untouched(out, energy, mixed)
    room[7] = -1
    assert call(K=64) == 0
    torch.cuda.synchronize()
    c = h.mix_count(cnt)
    assert c == dict(rows=n - 1, rooms=1, clipped=0)
    assert bool((out[7] == FILL_O).all()) and bool((out[:7] == 0).all()) and bool((out[n:] == FILL_O).all())
    h.close()


@need_ref
def test_gpu_bridge_against_the_compiled_reference(torch_cuda):
    """24 talkers in rooms of 2, 3, 3 and 16: encode -> send_pack (description loss) -> ring -> play-out -> mix(3) -> encode on a second
    handle; the reference codec per stream around the numpy model must give every payload byte and length record.  Each step runs once."""
    import solo_amd
    torch = torch_cuda
    N, P, FIRST = 24, 12, 700
    rates = [(9600, 12000, 13600)[i % 3] for i in range(N)]
    room = np.repeat(np.arange(4), (2, 3, 3, 16)).astype(np.int32)[np.random.default_rng(3).permutation(N)]
    x = np.stack([R.synth_stream(500 + i, P) for i in range(N)])
    rng = np.random.default_rng(17)
    send = rng.integers(0, 4, (N, P)).astype(np.uint8)
    send[rng.random((N, P)) < 0.6] = 3
    assert set(np.unique(send)) == {0, 1, 2, 3}

    def encoder():
        e = solo_amd.SoloBatch(N, rate=13600, encoder=True, decoder=False)
        e.reset_streams(list(range(N)), rate=rates, which="enc")
        return e

    tx = encoder()
    bits, nb, st = tx.encode(torch.from_numpy(x).cuda())
    rec, pay, cnt = tx.send_pack(bits, nb, send=torch.from_numpy(send).cuda(), first_seq=FIRST)
    c = tx.send_count(cnt)
    assert int(st.abs().max()) == 0 and int(nb[:, :, 0].max()) <= FRONT_END_BYTES and c["refused"] == 0 and c["records"] == c["records_needed"] > 0
    rx = solo_amd.SoloBatch(N, encoder=False, decoder=True)
    rx.recv_create(P, 256, 0)
    rx.recv_reset_streams(list(range(N)), FIRST)
    rx.recv_insert(rec[:c["records"]].contiguous(), pay)
    assert rx.recv_stats() == dict(inserted=c["records"], late=0, ahead=0, duplicate=0, bad=0)
    heard, st = rx.recv_decode(P)
    mixed_pcm, mcnt = rx.mix(heard, torch.from_numpy(room).cuda(), max_speakers=3)
    tx2 = encoder()
    bits2, nb2, st2 = tx2.encode(mixed_pcm)
    torch.cuda.synchronize()
    assert int(st.abs().max()) == 0 and int(st2.abs().max()) == 0 and rx.mix_count(mcnt)["rows"] == N
    hb, hn, hb2, hn2 = bits.cpu().numpy(), nb.cpu().numpy(), bits2.cpu().numpy(), nb2.cpu().numpy()

    ref_heard = np.zeros((N, P, 640), np.int16)
    for i in range(N):
        e, d = R.RefEncoder("fix", rate=rates[i]), R.RefDecoder("fix", use_md_index=0)
        for p in range(P):
            pl, n0, n1 = e.encode(x[i, p])
            assert hb[i, p, :n0].tobytes() == pl and (int(hn[i, p, 0]), int(hn[i, p, 1])) == (n0, n1), (i, p)
            m = int(send[i, p])
            ref_heard[i, p], ret = d.decode(*R.map_loss(pl, n0, n1, not m & 1, not m & 2))
            assert ret == 0
    assert np.array_equal(heard.cpu().numpy(), ref_heard)
    want = model_mix(ref_heard, room, 4, None, 3)
    assert 0 < want["mixed"][room == 3].sum() < 16 * P                                 # the room of 16 was cut to 3 speakers
    assert np.array_equal(mixed_pcm.cpu().numpy(), want["out"])
    for i in range(N):
        e = R.RefEncoder("fix", rate=rates[i])
        for p in range(P):
            pl, n0, n1 = e.encode(want["out"][i, p])
            assert (int(hn2[i, p, 0]), int(hn2[i, p, 1])) == (n0, n1) and hb2[i, p, :n0].tobytes() == pl, (i, rates[i], p)

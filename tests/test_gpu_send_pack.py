"""Sender back end on the GPU (solo_send_pack / solo_send_pack_streams through the binding and the C ABI): records, payload and counts
against the independent numpy model of tests/send_pack_model.py (mixed handles, poisoned length records, caps, 4096 x 50), and the
loopback encode -> pack -> solo_recv_insert -> solo_recv_decode against solo_batch_decode with the same mask on a fresh decoder, and
against the compiled reference decoder."""
import ctypes as C
import functools

import numpy as np
import pytest

import refcodec as R
import solo_testlib as T
from send_pack_model import INT32_MAX, model_pack

need_ref = pytest.mark.skipif(not R.have_ref("fix"), reason="oracle/_ref not present")
pytestmark = pytest.mark.gpu
FRONT_END_BYTES = 252            # what the receiver front end takes per packet (tests/test_gpu_rate_range.py pins it)
FILL_R, FILL_P = -7, 0xA5


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch


def _pcm(N, P, samplerate, framesize_ms, silent):
    """[N, P, samples]: 32 different signals, tiled; the rows in `silent` are zeros"""
    from solo_amd.synth import synth_stream
    L = 640 * samplerate // 16000 * framesize_ms // 40
    per40 = (samplerate // 16000) * P * framesize_ms // 40 + 2
    base = np.stack([synth_stream(900 + k, per40).reshape(-1)[:P * L].reshape(P, L) for k in range(32)])
    pcm = base[np.arange(N) % 32].copy()
    pcm[silent] = 0
    return pcm


@functools.lru_cache(maxsize=None)
def _encoded(N, P, samplerate, framesize_ms, safe, mdi="mixed", dtx=True):
    """One mixed handle encoded: several rates, some streams with DTX and silent input, useMDIndex 0 and 1 ->
    (bits, nbytes on the device, per-stream useMDIndex, hbb).  safe: rates whose packets the receiver front end takes."""
    import torch
    import solo_amd
    if samplerate == 16000:
        rates = [9600, 12000, 13600] if safe else [8000, 13600, 20000, 32000]
    else:
        rates = [20000, 24000] if safe else [16000, 24000, 32000, 40000]
    i = np.arange(N)
    rate = [rates[k % len(rates)] for k in i]
    md = [(k // 3) % 2 if mdi == "mixed" else int(mdi) for k in i]
    dtx_on = [bool(dtx) and k % 5 == 4 for k in i]
    enc = solo_amd.SoloBatch(N, rate=rates[-1], encoder=True, decoder=False, samplerate=samplerate, framesize_ms=framesize_ms)
    enc.reset_streams(list(range(N)), rate=rate, dtx=dtx_on, use_md_index=md, which="enc")
    pcm = _pcm(N, P, samplerate, framesize_ms, np.array(dtx_on))
    bits, nb, st = enc.encode(torch.from_numpy(pcm).cuda())
    torch.cuda.synchronize()
    assert int(st.abs().max()) == 0
    enc.close()
    return bits, nb, np.array(md), 4 if framesize_ms == 20 else 8


def _pack_and_compare(torch, h, bits, nb, send, seq_base, first_seq, hbb, streams=None, max_records=None, cap=None):
    """send_pack into guarded buffers; records, payload, count and the guards against the model.  -> (records, payload, count, model)"""
    n, P, slot = bits.shape
    mr = 2 * n * P if max_records is None else max_records
    cp = n * P * slot if cap is None else cap
    G = 64
    rec = torch.full((mr + G, 5), FILL_R, dtype=torch.int32, device="cuda")
    pay = torch.full((cp + G,), FILL_P, dtype=torch.uint8, device="cuda")
    r, p, cnt = h.send_pack(bits, nb, send=send, first_seq=first_seq, seq_base=seq_base, records=rec[:mr], payload=pay[:cp], streams=streams)
    c = h.send_count(cnt)
    want = model_pack(bits.cpu().numpy(), nb.cpu().numpy(), None if send is None else send.cpu().numpy(),
                      None if seq_base is None else seq_base.cpu().numpy(), first_seq, hbb,
                      None if streams is None else np.asarray(streams), mr, cp)
    print("send_pack %d x %d: count %s" % (n, P, c))
    assert c == want["count"], (c, want["count"])
    hr, hp = rec.cpu().numpy(), pay.cpu().numpy()
    assert np.array_equal(hr[:c["records"]], want["records"])
    assert np.array_equal(hp[:c["bytes"]], want["payload"])
    assert (hr[c["records"]:] == FILL_R).all() and (hp[c["bytes"]:] == FILL_P).all()      # nothing behind what was written, nor behind the caps
    return rec[:c["records"]], pay[:cp], c, want


def _poison(torch, nb, slot):
    """a few hand-made bad length records: each refusal reason of the length rules"""
    h = nb.cpu().numpy().copy()
    n, P = h.shape[:2]
    live = np.argwhere(h[:, :, 0] > 20)
    assert len(live) > 40
    for j, (why, (i, p)) in enumerate(zip(("big", "neg", "over", "short", "big", "neg", "over", "short"), live[3::5])):
        if why == "big":
            h[i, p, 0] = slot + 1
        elif why == "neg":
            h[i, p, 1] = -1 - j
        elif why == "over":
            h[i, p, 1] = h[i, p, 0] + 1
        else:
            h[i, p, 1] = 3
    return torch.from_numpy(h).cuda()


def _mask_and_seq(torch, n, P, seed, overflow=True):
    rng = np.random.default_rng(seed)
    send = rng.integers(0, 4, (n, P)).astype(np.uint8)
    send[rng.random((n, P)) < 0.5] = 3
    base = rng.integers(0, 100000, n).astype(np.int32)
    if overflow:
        base[1] = INT32_MAX - P // 2            # this stream's numbers run over the top inside the call
    return torch.from_numpy(send).cuda(), torch.from_numpy(base).cuda()


@pytest.mark.parametrize("samplerate,framesize_ms", [(16000, 40), (32000, 40), (16000, 20)])
def test_gpu_model_parity(torch_cuda, samplerate, framesize_ms):
    import solo_amd
    torch = torch_cuda
    N, P = 256, 12
    bits, nb, md, hbb = _encoded(N, P, samplerate, framesize_ms, False)
    nb = _poison(torch, nb, bits.shape[2])
    send, base = _mask_and_seq(torch, N, P, 11)
    # any handle of the geometry will do: here one that has only a decoder
    h = solo_amd.SoloBatch(N, encoder=False, decoder=True, samplerate=samplerate, framesize_ms=framesize_ms)
    _, _, c, want = _pack_and_compare(torch, h, bits, nb, send, base, 7, hbb)
    assert c["empty"] > 0 and c["refused"] >= 8 and c["records"] == c["records_needed"] > N * P // 2
    assert all(v > 0 for v in want["reasons"].values()), want["reasons"]
    # no mask, no sequence base
    _pack_and_compare(torch, h, bits, nb, None, None, 0, hbb)


def test_gpu_caps(torch_cuda):
    import solo_amd
    torch = torch_cuda
    N, P = 256, 12
    bits, nb, md, hbb = _encoded(N, P, 16000, 40, False)
    nb = _poison(torch, nb, bits.shape[2])
    send, base = _mask_and_seq(torch, N, P, 11)
    h = solo_amd.SoloBatch(N, encoder=True, decoder=False)
    _, _, full, want = _pack_and_compare(torch, h, bits, nb, send, base, 7, hbb)
    allr = want["all_records"]
    need_r, need_b = full["records_needed"], full["bytes_needed"]
    ks = [k for k in range(300, need_r) if allr[k, 2] == 1 and allr[k - 1, 2] == 0 and (allr[k, :2] == allr[k - 1, :2]).all()]
    kb = [k for k in range(300, need_r) if allr[k, 2] == 0]
    k_in, k_edge = ks[len(ks) // 2], kb[len(kb) // 3]
    for mr, cp in [(k_edge, need_b), (k_in, need_b), (need_r, int(allr[k_in, 3])), (need_r, int(allr[k_in, 3] + allr[k_in, 4] - 1)),
                   (need_r, int(allr[k_edge, 3])), (0, need_b), (need_r, 0), (0, 0), (k_in, int(allr[k_edge, 3])), (need_r, need_b)]:
        _, _, c, _ = _pack_and_compare(torch, h, bits, nb, send, base, 7, hbb, max_records=mr, cap=cp)
        assert c["records_needed"] == need_r and c["bytes_needed"] == need_b and c["empty"] == full["empty"] and c["refused"] == full["refused"]
        assert c["records"] <= mr and c["bytes"] <= cp
        if (mr, cp) != (need_r, need_b):
            assert c["records"] < need_r


def _decoders(solo_amd, N, samplerate, md, streams=None):
    d = solo_amd.SoloBatch(N, encoder=False, decoder=True, samplerate=samplerate)
    d.reset_streams(list(range(N)) if streams is None else list(streams), use_md_index=[int(v) for v in md], which="dec")
    return d


def _loopback(torch, samplerate, mdi, dtx=True, N=256, P=12):
    """encode -> pack with mask M -> ring -> play-out == decode(bits, nbytes, recv=M) on a fresh decoder; -> what the reference check needs"""
    import solo_amd
    bits, nb, md, hbb = _encoded(N, P, samplerate, 40, True, mdi, dtx)
    hn = nb.cpu().numpy()
    assert int(hn[:, :, 0].max()) <= FRONT_END_BYTES, int(hn[:, :, 0].max())          # every packet is one the front end takes
    send, base = _mask_and_seq(torch, N, P, 23, overflow=False)
    FIRST = 1000
    tx = solo_amd.SoloBatch(N, encoder=True, decoder=False, samplerate=samplerate, rate=24000)
    rec, pay, c, _ = _pack_and_compare(torch, tx, bits, nb, send, base, FIRST, hbb)
    assert c["refused"] == 0 and c["records"] == c["records_needed"] > 0
    if dtx:
        assert c["empty"] > 0
    want_dec = _decoders(solo_amd, N, samplerate, md)
    want, st = want_dec.decode(bits, nb, send)
    torch.cuda.synchronize()
    assert int(st.abs().max()) == 0
    want = want.cpu().numpy()
    for unknown_desc in ([False, True] if mdi == 1 else [False]):
        rx = _decoders(solo_amd, N, samplerate, md)
        rx.recv_create(P, 256, 0)
        rx.recv_reset_streams(list(range(N)), [FIRST + int(v) for v in base.cpu().numpy()])
        arr = rec.clone()
        if unknown_desc:
            arr[:, 2] = -1
        rx.recv_insert(arr.contiguous(), pay)
        stats = rx.recv_stats()
        assert stats == dict(inserted=c["records"], late=0, ahead=0, duplicate=0, bad=0), (stats, c)
        got, st = rx.recv_decode(P)
        torch.cuda.synchronize()
        assert int(st.abs().max()) == 0
        got = got.cpu().numpy()
        bad = np.argwhere((got != want).any(axis=2))
        assert len(bad) == 0, (unknown_desc, bad[:8].tolist())
    return bits.cpu().numpy(), hn, send.cpu().numpy(), want


@pytest.mark.parametrize("samplerate,mdi", [(16000, "mixed"), (16000, 1), (32000, 1), (32000, 0)])
def test_gpu_loopback_against_the_decoder(torch_cuda, samplerate, mdi):
    _loopback(torch_cuda, samplerate, mdi)


@need_ref
def test_gpu_loopback_against_the_compiled_reference(torch_cuda):
    N, P = 32, 12
    bits, hn, send, pcm = _loopback(torch_cuda, 16000, 0, dtx=False, N=N, P=P)
    rates = [9600, 12000, 13600]
    seen = set()
    for i in range(N):
        d = R.RefDecoder("fix", use_md_index=0)
        for p in range(P):
            n0, n1 = int(hn[i, p, 0]), int(hn[i, p, 1])
            assert n0 > 0
            m = int(send[i, p])
            x, ret = d.decode(*R.map_loss(bits[i, p, :n0].tobytes(), n0, n1, not m & 1, not m & 2))
            assert ret == 0 and np.array_equal(pcm[i, p], x), (i, rates[i % 3], p, m)
            seen.add(m)
    assert seen == {0, 1, 2, 3}


def test_gpu_subset_form(torch_cuda):
    import solo_amd
    torch = torch_cuda
    N, P = 64, 12
    lst = list(range(1, N, 2))
    n = len(lst)
    md = [(k // 3) % 2 for k in lst]
    enc = solo_amd.SoloBatch(N, rate=13600, encoder=True, decoder=False)
    enc.reset_streams(lst, rate=[(9600, 12000, 13600)[k % 3] for k in lst], use_md_index=md, which="enc")
    pcm = _pcm(n, P, 16000, 40, np.zeros(n, bool))
    bits, nb, st = enc.encode(torch.from_numpy(pcm).cuda(), streams=lst)
    torch.cuda.synchronize()
    assert int(st.abs().max()) == 0 and int(nb[:, :, 0].max()) <= FRONT_END_BYTES and int(nb[:, :, 0].min()) > 0
    send, base = _mask_and_seq(torch, n, P, 31, overflow=False)
    rec, pay, c, _ = _pack_and_compare(torch, enc, bits, nb, send, base, 50, 8, streams=lst)
    assert set(rec[:, 0].cpu().numpy().tolist()) == set(lst)              # slot indices, not rows
    want_dec = _decoders(solo_amd, N, 16000, md, lst)
    want, st = want_dec.decode(bits, nb, send, streams=lst)
    rx = _decoders(solo_amd, N, 16000, md, lst)
    rx.recv_create(P, 256, 0)
    rx.recv_reset_streams(lst, [50 + int(v) for v in base.cpu().numpy()])
    rx.recv_insert(rec.contiguous(), pay)
    assert rx.recv_stats() == dict(inserted=c["records"], late=0, ahead=0, duplicate=0, bad=0)
    got, st2 = rx.recv_decode(P, streams=lst)
    torch.cuda.synchronize()
    assert int(st.abs().max()) == 0 and int(st2.abs().max()) == 0
    assert np.array_equal(got.cpu().numpy(), want.cpu().numpy())
    # a list that is not increasing (the binding would refuse it: through the C ABI): records = -1, nothing else written
    bad = torch.tensor([3, 1] + lst[2:], dtype=torch.int32, device="cuda")
    r2 = torch.full((2 * n * P, 5), FILL_R, dtype=torch.int32, device="cuda")
    p2 = torch.full((n * P * 512,), FILL_P, dtype=torch.uint8, device="cuda")
    cnt = torch.full((8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    ret = enc.lib.solo_send_pack_streams(enc.h, bad.data_ptr(), n, bits.data_ptr(), nb.data_ptr(), send.data_ptr(), P, base.data_ptr(), 50,
                                         r2.data_ptr(), r2.shape[0], p2.data_ptr(), p2.shape[0], cnt.data_ptr(), enc._stream())
    torch.cuda.synchronize()
    assert ret == 0
    hc = cnt.cpu().numpy()
    assert hc[0] == -1 and (hc[1:] == 0x5A5A5A5A).all()
    assert enc.send_count(cnt)["records"] == -1
    assert bool((r2 == FILL_R).all()) and bool((p2 == FILL_P).all())
    # and the handle packs on afterwards
    _pack_and_compare(torch, enc, bits, nb, send, base, 50, 8, streams=lst)
    # host refusals of the C ABI on a live handle
    L = enc.lib
    args = lambda **k: [k.get("bits", bits.data_ptr()), nb.data_ptr(), None, k.get("P", P), None, 0, r2.data_ptr(), k.get("mr", 10), p2.data_ptr(),
                        k.get("cap", 10), k.get("cnt", cnt.data_ptr()), None]
    big = solo_amd.SoloBatch(N, encoder=False, decoder=True)
    assert L.solo_send_pack(big.h, *args(bits=None)) == -1 and L.solo_send_pack(big.h, *args(P=0)) == -1
    assert L.solo_send_pack(big.h, *args(mr=-1)) == -1 and L.solo_send_pack(big.h, *args(cap=-1)) == -1 and L.solo_send_pack(big.h, *args(cnt=None)) == -1
    assert L.solo_send_pack(big.h, *args(P=2 ** 31 // (2 * N))) == -1               # n * P * 2 = 2^31
    assert L.solo_send_pack_streams(big.h, bad.data_ptr(), 0, *args()) == -1 and L.solo_send_pack_streams(big.h, bad.data_ptr(), N + 1, *args()) == -1
    assert L.solo_send_pack_streams(big.h, None, n, *args()) == -1


def test_gpu_send_pack_4096_x_50(torch_cuda):
    """the size of the flagship workload: 800 tiles, thirteen rounds of the second-level scan, ~16 MB of payload"""
    import solo_amd
    torch = torch_cuda
    N, P = 4096, 50
    bits, nb, md, hbb = _encoded(N, P, 16000, 40, False)
    nb = _poison(torch, nb, bits.shape[2])
    send, base = _mask_and_seq(torch, N, P, 41)
    h = solo_amd.SoloBatch(N, encoder=False, decoder=True)
    _, _, c, _ = _pack_and_compare(torch, h, bits, nb, send, base, 3, hbb)
    assert c["records"] > N * P // 2 and c["bytes"] > 4 * 2 ** 20 and c["empty"] > 0 and c["refused"] > 0
    _encoded.cache_clear()

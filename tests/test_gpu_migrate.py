"""Stream migration on the GPU (solo_batch_export_streams / solo_batch_import_streams): a call that moves to another handle in the
middle goes on bit-exactly.  The expected outputs are the golden fixtures of test_gpu_encoder.py / test_gpu_decoder.py (synth8x25.npz,
wb4x20.npz for 32 kHz): the yardstick is the reference, not an uninterrupted run of the code under test.  The fixtures' own receive
mask is a 30 % Bernoulli loss of descriptions, so near a split it has isolated lost and single-description packets but no burst; the
mask made for the split -- a loss burst, an MD1-only run and an MD2-only run that straddle it -- has no fixture output and is checked
against the compiled reference in tests of its own (test_decoder_straddling_mask_vs_compiled_reference), which are skipped where
oracle/_ref is not present.  The encoder halves on the target handle are calls of more than one packet (k = 1, 7),
so under the persistent schedule (opt-in: SOLO_ENC_PERSIST=1; the default is the launch-per-chunk schedule) an imported stream would
encode with that schedule's per-handle words, which do not travel; k = 24 leaves one packet and with it the launch-per-chunk schedule
whatever the setting."""
import numpy as np
import pytest

import refcodec as R
import solo_testlib as T

pytestmark = pytest.mark.gpu
need_ref = pytest.mark.skipif(not R.have_ref("fix"), reason="oracle/_ref not present")
SRC, DST = [1, 4, 6], [0, 1, 2]
FIX = {16000: ("synth8x25.npz", dict()), 32000: ("wb4x20.npz", dict(rate=24000, samplerate=32000))}
# wb4x20.npz: rows 0 .. 2 are joint_mode 0 and can share a handle (row 1 starts with two lost packets), row 3 is joint_mode 1
WB_ROWS, WB_SRC, WB_DST = [0, 1, 2], [1, 2], [0, 2]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch


@pytest.fixture(scope="module")
def fixtures():
    return {fs: np.load(T.GOLDEN + "/" + name) for fs, (name, _) in FIX.items()}


def _batch(n, fs=16000, enc=True, dec=True, slot=512, **kw):
    import solo_amd
    return solo_amd.SoloBatch(n, encoder=enc, decoder=dec, slot_bytes=slot, **{**FIX[fs][1], **kw})


def _dev(b, x):
    return b.torch.from_numpy(np.ascontiguousarray(x)).to(b.device)


def _same_payload(bits, nb, zbits, znb):
    bits, nb = bits.cpu().numpy(), nb.cpu().numpy()
    assert np.array_equal(nb, znb)
    for i in range(nb.shape[0]):
        for p in range(nb.shape[1]):
            n = max(int(nb[i, p, 0]), 0)
            assert np.array_equal(bits[i, p, :n], zbits[i, p, :n]), (i, p)


def _move(a, b, src, dst, which):
    blob, c = a.export_streams(src, which)
    assert a.migrate_count(c) == dict(streams=len(src), refused=0, bytes=len(src) * a.state_bytes(which))
    c = b.import_streams(dst, blob, which)
    assert b.migrate_count(c) == dict(streams=len(dst), refused=0, bytes=len(dst) * b.state_bytes(which))
    return blob


def _rows(z, rows):
    """the fixture's streams `rows` alone: what one handle of their geometry holds"""
    return {name: z[name][rows] for name in z.files}


def _encoder_continuity(z, fs, src, k, dst=DST, joint=0, **b_ctrl):
    """z: the streams of handle A; `src` of them move into the slots `dst` of the three-stream handle B"""
    N, P, S = z["bits"].shape
    a, b = _batch(N, fs, dec=False, slot=S, joint=joint), _batch(3, fs, dec=False, slot=S, joint=joint, **b_ctrl)
    bits, nb, st = a.encode(_dev(a, z["pcm"][:, :k]))
    assert int(st.abs().max()) == 0
    _same_payload(bits, nb, z["bits"][:, :k], z["nbytes"][:, :k])
    _move(a, b, src, dst, "enc")
    bits, nb, st = b.encode(_dev(b, z["pcm"][src, k:]), streams=None if len(dst) == 3 else dst)
    assert int(st.abs().max()) == 0
    _same_payload(bits, nb, z["bits"][src, k:], z["nbytes"][src, k:])


@pytest.mark.parametrize("k", [1, 7, 24])
def test_encoder_continuity(torch_cuda, fixtures, k):
    _encoder_continuity(fixtures[16000], 16000, SRC, k)


def test_encoder_control_travels(torch_cuda, fixtures):
    """the target handle was created at another rate and with DTX on: the imported streams keep the control they were exported with"""
    _encoder_continuity(fixtures[16000], 16000, SRC, 7, rate=24000, dtx=1)


def _ref_decode(z, fs, stream, recv, joint=0):
    d = R.RefDecoder("fix", samplerate=fs, joint=joint)
    out = []
    for p in range(recv.shape[0]):
        n0, n1 = int(z["nbytes"][stream, p, 0]), int(z["nbytes"][stream, p, 1])
        m = int(recv[p])
        pay, a0, a1, flag = R.map_loss(z["bits"][stream, p, :n0].tobytes(), n0, n1, not (m & 1), not (m & 2))
        y, r = d.decode(pay, a0, a1, flag)
        assert r == 0
        out.append(y)
    return np.stack(out)


def _decoder_continuity(z, fs, src, k, recv, want, dst=DST, joint=0):
    """want: [N, P, L] for the mask `recv` [N, P]"""
    N, P, S = z["bits"].shape
    a, b = _batch(N, fs, enc=False, slot=S, joint=joint), _batch(3, fs, enc=False, slot=S, joint=joint)
    pcm, st = a.decode(_dev(a, z["bits"][:, :k]), _dev(a, z["nbytes"][:, :k]), _dev(a, recv[:, :k]))
    assert int(st.abs().max()) == 0 and np.array_equal(pcm.cpu().numpy(), want[:, :k])
    _move(a, b, src, dst, "dec")
    pcm, st = b.decode(_dev(b, z["bits"][src, k:]), _dev(b, z["nbytes"][src, k:]), _dev(b, recv[src, k:]), streams=None if len(dst) == 3 else dst)
    assert int(st.abs().max()) == 0 and np.array_equal(pcm.cpu().numpy(), want[src, k:])


def _straddling_mask(z, src, k):
    """a loss burst, an MD1-only run and an MD2-only run of four packets each around the split, one per moved stream"""
    recv = np.full(z["recv"].shape, 3, np.uint8)
    lo, hi = max(k - 2, 0), min(k + 2, recv.shape[1])
    for s, m in zip(src, (0, 1, 2)):
        recv[s, lo:hi] = m
    return recv


def _decoder_case(z, fs, src, k, dst=DST, joint=0):
    """the fixture's own mask (30 % description loss, no burst) against the fixture's reference output"""
    _decoder_continuity(z, fs, src, k, z["recv"], z["dec_loss"], dst, joint)


def _decoder_straddle(z, fs, src, k, dst=DST, joint=0):
    """a mask made for the split, against the compiled reference (the other streams receive everything: dec_clean)"""
    recv = _straddling_mask(z, src, k)
    want = z["dec_clean"].copy()
    for s in src:
        want[s] = _ref_decode(z, fs, s, recv[s], joint)
    _decoder_continuity(z, fs, src, k, recv, want, dst, joint)


@pytest.mark.parametrize("k", [1, 7, 24])
def test_decoder_continuity(torch_cuda, fixtures, k):
    _decoder_case(fixtures[16000], 16000, SRC, k)


def test_32khz_continuity(torch_cuda, fixtures):
    """a handle has one joint mode, so the fixture's joint_mode 0 rows share handle A and two of them move"""
    z = _rows(fixtures[32000], WB_ROWS)
    _encoder_continuity(z, 32000, WB_SRC, 7, WB_DST)
    _decoder_case(z, 32000, WB_SRC, 7, WB_DST)


def test_32khz_joint_continuity(torch_cuda, fixtures):
    """the fixture's joint_mode 1 row, from a handle of its own into the middle slot of a three-stream handle"""
    z = _rows(fixtures[32000], [3])
    _encoder_continuity(z, 32000, [0], 7, [1], joint=1)
    _decoder_case(z, 32000, [0], 7, [1], joint=1)


@need_ref
@pytest.mark.parametrize("case", ["16k_k1", "16k_k7", "16k_k24", "32k", "32k_joint"])
def test_decoder_straddling_mask_vs_compiled_reference(torch_cuda, fixtures, case):
    """a loss burst, an MD1-only run and an MD2-only run across the split, one per moved stream"""
    if case.startswith("16k"):
        _decoder_straddle(fixtures[16000], 16000, SRC, int(case[5:]))
    elif case == "32k":
        _decoder_straddle(_rows(fixtures[32000], WB_ROWS), 32000, WB_SRC, 7, WB_DST)
    else:
        _decoder_straddle(_rows(fixtures[32000], [3]), 32000, [0], 7, [1], joint=1)


def test_neighbours_and_identity(torch_cuda, fixtures):
    torch = torch_cuda
    z = fixtures[16000]
    N, P, S = z["bits"].shape
    a, b = _batch(N, slot=S), _batch(5, slot=S)
    k = 7
    a.encode(_dev(a, z["pcm"][:, :k]))
    a.decode(_dev(a, z["bits"][:, :k]), _dev(a, z["nbytes"][:, :k]), _dev(a, z["recv"][:, :k]))
    b.encode(_dev(b, z["pcm"][:5, :3]))                      # (B's own streams have a history as well)
    # an unlisted slot of B is byte-equal before and after an import
    before, _ = b.export_streams([1, 3])
    blob = _move(a, b, SRC, [0, 2, 4], "both")
    after, _ = b.export_streams([1, 3])
    assert torch.equal(before, after)
    # export, import into the same slots, export again: equal blobs; and what B holds is what A sent (all but the origin word)
    again, _ = b.export_streams([0, 2, 4])
    assert torch.equal(again[:, 16:], blob[:, 16:])
    assert again[:, 12:16].cpu().numpy().view(np.int32).reshape(-1).tolist() == [0, 2, 4]
    c = b.import_streams([0, 2, 4], again)
    assert b.migrate_count(c)["streams"] == 3
    third, _ = b.export_streams([0, 2, 4])
    assert torch.equal(third, again)
    # the exports changed nothing: A goes on as the fixture says, for every stream
    bits, nb, st = a.encode(_dev(a, z["pcm"][:, k:]))
    _same_payload(bits, nb, z["bits"][:, k:], z["nbytes"][:, k:])
    pcm, st = a.decode(_dev(a, z["bits"][:, k:]), _dev(a, z["nbytes"][:, k:]), _dev(a, z["recv"][:, k:]))
    assert np.array_equal(pcm.cpu().numpy(), z["dec_loss"][:, k:])
    # and so do the moved streams on B, both directions at once
    bits, nb, st = b.encode(_dev(b, z["pcm"][SRC, k:]), streams=[0, 2, 4])
    _same_payload(bits, nb, z["bits"][SRC, k:], z["nbytes"][SRC, k:])
    pcm, st = b.decode(_dev(b, z["bits"][SRC, k:]), _dev(b, z["nbytes"][SRC, k:]), _dev(b, z["recv"][SRC, k:]), streams=[0, 2, 4])
    assert np.array_equal(pcm.cpu().numpy(), z["dec_loss"][SRC, k:])


def _arrivals(z, items):
    """items: (stream, seq, packet, descs) -> the arrival records and the payload pool of solo_recv_insert"""
    recs, pool, off = [], [], 0
    for s, seq, p, descs in items:
        n0, n1 = int(z["nbytes"][s, p, 0]), int(z["nbytes"][s, p, 1])
        for d in descs:
            pay = z["bits"][s, p, :n0 - n1] if d == 0 else z["bits"][s, p, n0 - n1:n0]
            recs.append((s, seq, d, off, pay.size))
            pool.append(pay)
            off += pay.size
    return np.array(recs, np.int32), np.concatenate(pool)


def test_receive_queue_travels(torch_cuda, fixtures):
    torch = torch_cuda
    z = fixtures[16000]
    N, P, S = z["bits"].shape
    D = 8
    a, b = _batch(N, enc=False, slot=S), _batch(3, enc=False, slot=S)
    for h, first in ((a, 0), (b, 40)):
        h.recv_create(D, 256, first)
        h.recv_track(True)
    ins = lambda h, items: h.recv_insert(*[_dev(h, x) for x in _arrivals(z, items)])
    ins(a, [(s, p, p, (0, 1)) for s in range(N) for p in range(3)])
    pcm, st = a.recv_decode(3)
    assert np.array_equal(pcm.cpu().numpy(), z["dec_clean"][:, :3])
    # play = 3: sequence numbers 8 .. 10 now live in the entries that 0 .. 2 left.  Both descriptions, a single one, a hole, one far
    # ahead in wrapped storage, one beyond the window (dropped and counted), a second copy (dropped and counted)
    ins(a, [(s, 3, 3, (0, 1)) for s in range(N)] + [(s, 4, 4, (s & 1,)) for s in range(N)] + [(s, 6, 6, (1, 0)) for s in range(N)] +
           [(s, 10, 10, (0, 1)) for s in range(N)] + [(s, 11, 11, (0,)) for s in range(N)] + [(s, 3, 3, (1,)) for s in SRC])
    # something else in B's ring and counters that the import must replace
    ins(b, [(s, 41, 2, (0,)) for s in range(3)])
    stats_before = b.recv_stats()
    _move(a, b, SRC, DST, "dec+recv")
    assert b.recv_stats() == stats_before
    ra, rb = a.recv_report(SRC)[0].cpu().numpy(), b.recv_report(DST)[0].cpu().numpy()
    assert np.array_equal(ra, rb)
    cols = dict(zip(a.RECV_REPORT, ra[0].tolist()))
    assert (cols["play"], cols["queued"], cols["complete"], cols["ready"], cols["span"], cols["head"]) == (3, 4, 3, 2, 8, 3)
    assert (cols["inserted"], cols["ahead"], cols["duplicate"], cols["played_both"]) == (13, 1, 1, 3)
    pa, sa = a.recv_decode(8, streams=SRC)
    pb, sb = b.recv_decode(8)
    assert torch.equal(pa, pb) and torch.equal(sa, sb) and int(sa.abs().max()) == 0
    assert np.array_equal(pa.cpu().numpy()[:, 0], z["dec_clean"][SRC, 3])        # (packet 3 arrived whole)
    assert np.array_equal(a.recv_report(SRC)[0].cpu().numpy(), b.recv_report(DST)[0].cpu().numpy())
    assert b.recv_stats() == stats_before


def _refused(b, dst, blob, which, rec):
    before, _ = b.export_streams(list(range(b.n_streams)), which if isinstance(which, str) else "both")
    need = b.state_bytes(which)
    if blob.shape[1] < need:                                 # (a stride the host accepts: the refusal under test is the device's)
        wide = b.torch.zeros((blob.shape[0], need), dtype=blob.dtype, device=blob.device)
        wide[:, :blob.shape[1]] = blob
        blob = wide
    c = b.migrate_count(b.import_streams(dst, blob, which))
    assert c == dict(streams=-1, refused=rec, bytes=0), c
    after, _ = b.export_streams(list(range(b.n_streams)), which if isinstance(which, str) else "both")
    assert b.torch.equal(before, after)


def test_refusals(torch_cuda, fixtures):
    torch = torch_cuda
    z = fixtures[16000]
    N, P, S = z["bits"].shape
    a = _batch(N, slot=S)
    a.encode(_dev(a, z["pcm"][:, :2]))
    a.recv_create(8, 256, 0)
    blob, _ = a.export_streams(SRC, "both")
    # a 16 kHz blob into a 32 kHz handle
    _refused(_batch(3, 32000, slot=S), DST, blob, "both", 1)
    # framesize_ms 20 against 40
    _refused(_batch(3, slot=S, framesize_ms=20), DST, blob, "both", 1)
    # ring depth 8 against 4
    qblob, _ = a.export_streams(SRC, "dec+recv")
    b4 = _batch(3, enc=False, slot=S)
    b4.recv_create(4, 256, 0)
    _refused(b4, DST, qblob, "dec+recv", 1)
    b = _batch(3, slot=S)
    # one corrupted body byte (third record), a wrong magic (second record)
    bad = blob.clone()
    bad[2, 64 + 5000] ^= 1
    _refused(b, DST, bad, "both", 3)
    bad = blob.clone()
    bad[1, 0] ^= 0x40
    _refused(b, DST, bad, "both", 2)
    # a list that is not increasing: the position is the record; an export with it writes streams = -1 and nothing else
    lst = torch.tensor([0, 2, 2], dtype=torch.int32, device=b.device)
    _refused(b, lst, blob, "both", 3)
    out = torch.full_like(blob, 0x5A)
    _, c = b.export_streams(lst, "both", blob=out)
    assert b.migrate_count(c)["streams"] == -1 and bool((out == 0x5A).all())
    # the untouched blob is accepted after all that
    assert b.migrate_count(b.import_streams(DST, blob, "both"))["streams"] == 3
    # host refusals: a stride that is too small, a direction the handle lacks, an unaligned stride, no list
    lib, cnt = b.lib, torch.zeros(4, dtype=torch.int32, device=b.device)
    ok = torch.tensor(DST, dtype=torch.int32, device=b.device)
    need = b.state_bytes("both")
    call = lambda f, h, w, stride, lp=None: f(h.h, ok.data_ptr() if lp is None else lp, 3, w, blob.data_ptr(), stride, cnt.data_ptr(), None)
    for f in (lib.solo_batch_export_streams, lib.solo_batch_import_streams):
        assert call(f, b, 3, need - 16) == -1
        assert call(f, b, 3, need + 8) == -1
        assert call(f, b, 0, need) == -1 and call(f, b, 8, need) == -1 and call(f, b, 4, need) == -1      # (no ring on b)
        assert call(f, b4, 1, need) == -1                            # which = 1 on a decoder-only handle
        assert call(f, b, 3, need, 0) == -1
    assert lib.solo_batch_state_bytes(b4.h, 1) == -1 and lib.solo_batch_state_bytes(b.h, 4) == -1
    assert need == blob.shape[1] and need % 16 == 0
    torch.cuda.synchronize()
    assert cnt.cpu().numpy().tolist() == [0, 0, 0, 0]                # nothing was enqueued

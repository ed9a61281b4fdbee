"""Read side of the receiver ring on the GPU (solo_recv_track, solo_recv_report), through the C ABI, against the independent model of
tests/recv_report_model.py.

The play-out simulation closes the loop the calls exist for: per tick the arrivals are filed, every stream is reported, the device-built
play-out list goes straight into solo_recv_decode_streams.  After EVERY tick all 16 fields of all streams, the list, the rows and the
count must equal the model, and the PCM of every played packet must equal the compiled reference decoder called with exactly what the
model says was queued.  The schedule (delays, losses, copies, arrivals far ahead, bad fields) does not depend on the payload bytes, so the
seed is checked ON THE MODEL ALONE, without a GPU, to reach every category the counters and the selection know."""
import ctypes as C

import numpy as np
import pytest

import refcodec as R
import solo_testlib as T
from recv_report_model import BAD, FIELDS, INSERTED, RingModel

SEED = 2024
N_SIM, P_SIM, D_SIM, SLOT_SIM, MAX_SPAN_SIM = 64, 18, 8, 256, 6


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch


def _as_i32(rep):
    return (rep & 0xFFFFFFFF).astype(np.uint32).view(np.int32).reshape(rep.shape)


# ---------------------------------------------------------------------------------------------------------------------
# the schedule of the simulation: which description arrives in which tick -- no payload bytes in here
# ---------------------------------------------------------------------------------------------------------------------
def _schedule(seed, N, P, D, slot, mdi):
    """-> (ticks: per tick a list of (stream, seq, desc, part, len_override), min_ready [N]).  part = (stream, packet, description) of the
    payload the arrival carries; len_override None = the part's own length.  Packet p is sent in tick p; a description arrives
    `delay` ticks later, or never, or twice; some arrivals carry a sequence number far ahead; some carry fields that must be refused."""
    rng = np.random.default_rng(seed)
    delay = rng.integers(0, 4, (N, P, 2)) + np.where(rng.random((N, P, 2)) < 0.08, 5, 0)
    lost = (rng.random((N, P, 2)) < 0.12) | (rng.random((N, P, 1)) < 0.10)           # one description, or the whole packet
    twice = rng.random((N, P, 2)) < 0.1
    ticks = [[] for _ in range(P)]
    for i in range(N):
        for p in range(P):
            for d in (0, 1):
                if lost[i, p, d]:
                    continue
                for k in range(2 if twice[i, p, d] else 1):
                    t = p + int(delay[i, p, d]) + k
                    if t < P:
                        ticks[t].append((i, p, -1 if mdi else d, (i, p, d), None))
    for t in range(P):
        for _ in range(6):
            i, p, d = int(rng.integers(0, N)), int(rng.integers(0, P)), int(rng.integers(0, 2))
            kind = int(rng.integers(0, 8))
            part = (i, p, d)
            ticks[t].append([(i, t + 1000, d, part, None),      # far ahead of any queue
                             (i, p, 2, part, None),             # no such description
                             (i, p, d, part, 0),                # empty
                             (i, p, d, part, slot + 1),         # larger than a slot
                             (i, -1, d, part, None),            # negative sequence number
                             (N, p, d, part, None),             # no such stream: counted in the handle's statistics only
                             (-1, p, d, part, None),
                             (i, p, d, part, -5)][kind])
        order = rng.permutation(len(ticks[t]))
        ticks[t] = [ticks[t][k] for k in order]
    min_ready = rng.integers(0, 4, N).astype(np.int32)
    return ticks, min_ready


def _arrivals(tick, parts):
    """rows (stream, seq, desc, offset, len) of a tick, given where each part lies in the payload pool"""
    out = []
    for s, seq, d, part, ln in tick:
        off, plen = parts[part]
        out.append((s, seq, d, off, plen if ln is None else ln))
    return out


def _simulate(ticks, min_ready, N, D, slot, mdi, parts, payload_bytes, step=None):
    """The model's side of the simulation; step(t, arrivals, model report, list, rows, played) is the GPU's turn, if any.
    -> (model, categories reached)"""
    m = RingModel(N, D, slot)
    m.track(True)
    true_desc = {off: part[2] for part, (off, _) in parts.items()}
    cat = dict(margin0=0, margin_pos=0, by_ready=0, by_span=0, not_selected=0)
    for t, tick in enumerate(ticks):
        arr = _arrivals(tick, parts)
        m.insert(arr, payload_bytes, [mdi] * N, true_desc)
        clear = t % 3 == 0
        rep, lst, rows = m.report(None, min_ready.tolist(), MAX_SPAN_SIM, clear_margin=clear)
        cat["margin0"] += int((rep[:, 15] == 0).sum())
        cat["margin_pos"] += int(((rep[:, 15] > 0) & (rep[:, 15] < D)).sum())
        for i in range(N):
            by_ready = rep[i, 3] >= min_ready[i]
            cat["by_ready"] += int(by_ready)
            cat["by_span"] += int(not by_ready and i in rows)
            cat["not_selected"] += int(i not in rows)
        played = m.play_out(lst, 1)
        if step:
            step(t, arr, rep, lst, rows, played, clear)
    tot = np.array(m.cnt).sum(axis=0)
    for k, name in enumerate(FIELDS[6:15]):
        cat[name] = int(tot[k])
    return m, cat


def _fake_parts(N, P):
    parts, off = {}, 0
    for i in range(N):
        for p in range(P):
            for d in (0, 1):
                parts[(i, p, d)] = (off, 40)
                off += 40
    return parts, off


@pytest.mark.parametrize("mdi", [0, 1])
def test_simulation_seed_reaches_every_category(mdi):
    """on the model alone (no GPU, no payload): the schedule of the GPU test below reaches every verdict, every play class, margins of 0
    and above, and all three outcomes of the selection -- each at least once per 64 streams"""
    ticks, min_ready = _schedule(SEED + mdi, N_SIM, P_SIM, D_SIM, SLOT_SIM, mdi)
    parts, pb = _fake_parts(N_SIM, P_SIM)
    m, cat = _simulate(ticks, min_ready, N_SIM, D_SIM, SLOT_SIM, mdi, parts, pb)
    assert all(v >= N_SIM // 64 for v in cat.values()), cat
    assert max(m.play) <= P_SIM                                # (no stream plays a packet that was never sent)
    assert m.stats[BAD] > cat["bad"]                           # (arrivals for streams that do not exist)


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def _encode_pool(torch, n_src, P, mdi, samplerate):
    """n_src streams x P packets encoded on the device -> (payload pool on the device, parts {(src, p, d): (offset, len)},
    recs [src][p] = (packet bytes, n0, n1), rate)"""
    import solo_amd
    if samplerate == 16000:
        pcm, rate = np.stack([R.synth_stream(700 + i, P) for i in range(n_src)]), 13600
    else:
        pcm, rate = np.stack([T.synth_stream_32k(700 + i, P) for i in range(n_src)]), 24000
    e = solo_amd.SoloBatch(n_src, rate=rate, encoder=True, decoder=False, slot_bytes=512, use_md_index=mdi, samplerate=samplerate)
    bits, nb, st = e.encode(torch.from_numpy(pcm).cuda())
    torch.cuda.synchronize()
    assert int(st.abs().max()) == 0
    hb, hn = bits.cpu().numpy(), nb.cpu().numpy()
    e.close()
    parts, recs, blobs, off = {}, [], [], 0
    for i in range(n_src):
        recs.append([])
        for p in range(P):
            n0, n1 = int(hn[i, p, 0]), int(hn[i, p, 1])
            pl = hb[i, p, :n0].tobytes()
            recs[i].append((pl, n0, n1))
            for d, part in enumerate((pl[:n0 - n1], pl[n0 - n1:])):
                assert 0 < len(part) <= SLOT_SIM
                parts[(i, p, d)] = (off, len(part))
                blobs.append(part)
                off += len(part)
    payload = torch.from_numpy(np.frombuffer(b"".join(blobs), np.uint8).copy()).cuda()
    return payload, parts, recs, rate


def _play_out_simulation(torch, mdi, samplerate=16000):
    import solo_amd
    N, P, D = N_SIM, P_SIM, D_SIM
    ticks, min_ready = _schedule(SEED + mdi, N, P, D, SLOT_SIM, mdi)
    # the seed's coverage, on the model alone, before anything runs on the device
    fake, fake_pb = _fake_parts(N, P)
    _, cat = _simulate(ticks, min_ready, N, D, SLOT_SIM, mdi, fake, fake_pb)
    assert all(v >= N // 64 for v in cat.values()), cat

    payload, parts, recs, rate = _encode_pool(torch, N, P, mdi, samplerate)
    b = solo_amd.SoloBatch(N, rate=rate, encoder=False, decoder=True, slot_bytes=512, use_md_index=mdi, samplerate=samplerate)
    b.recv_create(D, SLOT_SIM, 0)
    b.recv_track(True)
    d_min_ready = torch.from_numpy(min_ready).cuda()
    stats0 = b.recv_stats()
    played_pcm = [[] for _ in range(N)]                        # per stream: (seq, [arrival A, arrival B], pcm)

    def step(t, arr, rep, lst, rows, played, clear):
        b.recv_insert(torch.tensor(arr, dtype=torch.int32).cuda(), payload)
        g_rep, g_lst, g_rows, g_cnt = b.recv_report(min_ready=d_min_ready, max_span=MAX_SPAN_SIM, clear_margin=clear)
        cnt = b.recv_report_count(g_cnt)
        assert cnt == {"selected": len(lst), "listed": N}, (t, cnt, len(lst))
        got = g_rep.cpu().numpy()
        want = _as_i32(rep)
        if not np.array_equal(got, want):
            i, k = np.argwhere(got != want)[0]
            raise AssertionError("tick %d stream %d field %s: %d, model %d" % (t, i, FIELDS[k], got[i, k], want[i, k]))
        assert g_lst.cpu().numpy()[:len(lst)].tolist() == lst and g_rows.cpu().numpy()[:len(rows)].tolist() == rows, t
        if lst:
            pcm, st = b.recv_decode(1, streams=g_lst[:len(lst)])
            torch.cuda.synchronize()
            assert int(st.abs().max()) == 0, (t, st.cpu().numpy().tolist())
            x = pcm.cpu().numpy()
            for k, s in enumerate(lst):
                seq, src = played[k][0]
                played_pcm[s].append((seq, src, x[k, 0]))

    m, cat2 = _simulate(ticks, min_ready, N, D, SLOT_SIM, mdi, parts, int(payload.numel()), step)
    assert cat2 == cat                                         # (the real lengths change no verdict)
    # after the last tick: the counters once more, and their sums against the handle's statistics
    g_rep = b.recv_report()[0].cpu().numpy()
    assert np.array_equal(g_rep, _as_i32(m.report()[0]))
    stats = b.recv_stats()
    tot = g_rep[:, 6:11].astype(np.int64).sum(axis=0)
    for k, name in enumerate(("inserted", "late", "ahead", "duplicate")):
        assert stats[name] - stats0[name] == int(tot[k]) == m.stats[k] > 0, (name, stats, tot)
    assert stats["bad"] == m.stats[BAD] and stats["bad"] > int(tot[4]) > 0
    assert int(g_rep[:, 11:15].sum()) == sum(len(x) for x in played_pcm) > 0
    b.close()
    if not R.have_ref("fix"):
        pytest.skip("oracle/_ref not present: compared with the model only")
    classes = set()
    for i in range(N):
        dr = R.RefDecoder("fix", use_md_index=mdi, samplerate=samplerate)
        for seq, (sa, sb), x in played_pcm[i]:
            pl, n0, n1 = recs[i][seq]
            # what was queued is what was sent: description d of packet (i, seq), whole
            assert sa in (None, parts[(i, seq, 0)]) and sb in (None, parts[(i, seq, 1)])
            want, ret = dr.decode(*R.map_loss(pl, n0, n1, sa is None, sb is None))
            assert ret == 0 and np.array_equal(x, want), (i, seq, sa, sb)
            classes.add((sa is None, sb is None))
    assert len(classes) == 4


@pytest.mark.gpu
@pytest.mark.parametrize("mdi", [0, 1])
def test_gpu_play_out_simulation(torch_cuda, mdi):
    _play_out_simulation(torch_cuda, mdi)


@pytest.mark.gpu
def test_gpu_play_out_simulation_32k(torch_cuda):
    _play_out_simulation(torch_cuda, 1, samplerate=32000)


def _small_ring(torch, N, D, n_src=4, P=6, track=None, samplerate=16000):
    """a handle with a ring and a pool of real descriptions; arrivals(lst of (stream, seq, d)) files part (stream % n_src, seq % P, d)"""
    import solo_amd
    payload, parts, recs, rate = _encode_pool(torch, n_src, P, 0, samplerate)
    b = solo_amd.SoloBatch(N, rate=rate, encoder=False, decoder=True, slot_bytes=512, samplerate=samplerate)
    b.recv_create(D, SLOT_SIM, 0)
    if track is not None:
        b.recv_track(track)

    def rows(lst):
        return [(s, q, d) + parts[(s % n_src, q % P, d)] for s, q, d in lst]
    return b, payload, rows


def _file(torch, b, m, payload, arr):
    b.recv_insert(torch.tensor(arr, dtype=torch.int32).cuda(), payload)
    if m is not None:
        m.insert(arr, int(payload.numel()), [0] * m.N, {})


@pytest.mark.gpu
def test_gpu_tracking_off_changes_nothing(torch_cuda):
    """the same arrivals into a handle that tracks and one that does not: PCM, status, statistics and queue fields identical; the
    counters of the one that does not read 0, its margin_min the depth"""
    torch = torch_cuda
    N, D, P = 24, 4, 8
    rng = np.random.default_rng(5)
    out = []
    for track in (None, True):
        b, payload, rows = _small_ring(torch, N, D, P=P, track=track)
        rng = np.random.default_rng(5)
        res = []
        for t in range(P):
            arr = rows([(s, t + int(rng.integers(-1, 3)), int(rng.integers(0, 2))) for s in range(N) for _ in range(2) if rng.random() < 0.8])
            arr = [a for a in arr if a[1] >= 0]
            b.recv_insert(torch.tensor(arr, dtype=torch.int32).cuda(), payload)
            rep = b.recv_report()[0].cpu().numpy()
            pcm, st = b.recv_decode(1)
            torch.cuda.synchronize()
            res.append((rep, pcm.cpu().numpy(), st.cpu().numpy()))
        out.append((res, b.recv_stats()))
        b.close()
    (off, stats_off), (on, stats_on) = out
    assert stats_off == stats_on and stats_on["late"] > 0 and stats_on["duplicate"] > 0
    for (r0, p0, s0), (r1, p1, s1) in zip(off, on):
        assert np.array_equal(r0[:, :6], r1[:, :6]) and np.array_equal(p0, p1) and np.array_equal(s0, s1)
        assert (r0[:, 6:15] == 0).all() and (r0[:, 15] == D).all()
    assert on[-1][0][:, 6:15].sum() > 0 and (on[-1][0][:, 15] < D).any()


def _raw_report(b, torch, d_streams, n, rep, lst, rows, cnt, flags=0, min_ready=1, max_span=0, d_min_ready=None):
    ptr = lambda x: x.data_ptr() if x is not None else None
    return b.lib.solo_recv_report(b.h, ptr(d_streams), n, ptr(d_min_ready), min_ready, max_span, flags, ptr(rep), ptr(lst), ptr(rows), ptr(cnt),
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.mark.gpu
def test_gpu_subset_and_refusals(torch_cuda):
    torch = torch_cuda
    N, D = 16, 8
    b, payload, rows = _small_ring(torch, N, D, track=True)
    m = RingModel(N, D, SLOT_SIM)
    m.track(True)
    _file(torch, b, m, payload, rows([(s, 1 + s % 3, s & 1) for s in range(N)] + [(s, 0, 0) for s in range(0, N, 2)]))
    dev = lambda x: torch.tensor(x, dtype=torch.int32).cuda()
    PAT = -0x12345678
    fresh = lambda: (torch.full((N, 16), PAT, dtype=torch.int32).cuda(), torch.full((N,), PAT, dtype=torch.int32).cuda(),
                     torch.full((N,), PAT, dtype=torch.int32).cuda(), torch.full((2,), PAT, dtype=torch.int32).cuda())
    # a strict subset with CLEAR_MARGIN: the unlisted streams keep their margins
    sub = [1, 2, 5, 8, 9, 15]
    rep, lst, rws, cnt = fresh()
    assert _raw_report(b, torch, dev(sub), len(sub), rep, lst, rws, cnt, flags=1) == 0
    w_rep, w_lst, w_rows = m.report(sub, 1, 0, clear_margin=True)
    k = len(w_lst)
    assert cnt.cpu().numpy().tolist() == [k, len(sub)] and 0 < k < len(sub)
    assert np.array_equal(rep.cpu().numpy()[:len(sub)], _as_i32(w_rep)) and (rep.cpu().numpy()[len(sub):] == PAT).all()
    assert lst.cpu().numpy()[:k].tolist() == w_lst and rws.cpu().numpy()[:k].tolist() == w_rows
    assert (lst.cpu().numpy()[k:] == PAT).all() and (rws.cpu().numpy()[k:] == PAT).all()
    full = b.recv_report()[0].cpu().numpy()
    assert np.array_equal(full, _as_i32(m.report()[0]))
    assert (full[sub, 15] == D).all() and (np.delete(full, sub, axis=0)[:, 15] < D).all()
    # lists the device refuses: selected = -1, nothing else written, no margin cleared
    before = b.recv_report()[0].cpu().numpy()
    for bad in ([3, 3], [4, 2], [0, N], [-1, 3], [0, 1, 2, 7, 6]):
        rep, lst, rws, cnt = fresh()
        assert _raw_report(b, torch, dev(bad), len(bad), rep, lst, rws, cnt, flags=1, min_ready=0) == 0
        torch.cuda.synchronize()
        assert cnt.cpu().numpy().tolist() == [-1, PAT], bad
        assert (rep.cpu().numpy() == PAT).all() and (lst.cpu().numpy() == PAT).all() and (rws.cpu().numpy() == PAT).all(), bad
        assert np.array_equal(b.recv_report()[0].cpu().numpy(), before), bad
        # ... and a refused play-out list plays and counts nothing
        pcm, st = torch.zeros((len(bad), 1, 640), dtype=torch.int16).cuda(), torch.zeros(len(bad), dtype=torch.int32).cuda()
        assert b.lib.solo_recv_decode_streams(b.h, dev(bad).data_ptr(), len(bad), 1, pcm.data_ptr(), st.data_ptr(),
                                              C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
        assert (st.cpu().numpy() == -1).all()
        assert np.array_equal(b.recv_report()[0].cpu().numpy(), before), bad
    # what the host refuses: -1, nothing enqueued
    rep, lst, rws, cnt = fresh()
    one = dev([0])
    refused = [
        _raw_report(b, torch, None, 0, rep, lst, rws, cnt), _raw_report(b, torch, one, 0, rep, lst, rws, cnt), _raw_report(b, torch, one, -1, rep, lst, rws, cnt),
        _raw_report(b, torch, one, N + 1, rep, lst, rws, cnt), _raw_report(b, torch, None, N - 1, rep, lst, rws, cnt),
        _raw_report(b, torch, None, N, None, None, None, cnt), _raw_report(b, torch, None, N, None, None, None, None),
        _raw_report(b, torch, None, N, rep, lst, None, None), _raw_report(b, torch, None, N, None, None, rws, None),
        _raw_report(b, torch, None, N, rep, lst, rws, cnt, flags=2), _raw_report(b, torch, None, N, rep, lst, rws, cnt, flags=-1),
        _raw_report(b, torch, None, N, rep[0, 1:], lst, rws, cnt),                      # a record array that is not 16-byte aligned
    ]
    assert refused == [-1] * len(refused), refused
    torch.cuda.synchronize()
    assert (rep.cpu().numpy() == PAT).all() and (cnt.cpu().numpy() == PAT).all()
    # the reports alone need no count; a count comes with the reports alone when asked for
    assert _raw_report(b, torch, None, N, rep, None, None, None) == 0
    assert _raw_report(b, torch, None, N, rep, None, None, cnt) == 0
    assert cnt.cpu().numpy().tolist() == [len(m.report(None, 1, 0)[1]), N]
    # a handle without a ring
    import solo_amd
    b2 = solo_amd.SoloBatch(4, encoder=False, decoder=True)
    assert b2.lib.solo_recv_track(b2.h, 1, None) == -1
    assert _raw_report(b2, torch, None, 4, rep, lst, rws, cnt) == -1
    b2.close()
    b.close()


@pytest.mark.gpu
def test_gpu_counter_lifecycle(torch_cuda):
    """recv_reset_streams zeroes the listed streams' counters only, recv_create those of all streams, recv_track(0) freezes them (and
    the next recv_track(1) starts from zero)"""
    torch = torch_cuda
    N, D = 12, 4
    b, payload, rows = _small_ring(torch, N, D, track=True)
    m = RingModel(N, D, SLOT_SIM)
    m.track(True)

    def tick(t):
        _file(torch, b, m, payload, rows([(s, t + (s % 3) - 1, s & 1) for s in range(N) if t + (s % 3) - 1 >= 0]))
        b.recv_decode(1)
        m.play_out(range(N), 1)

    def check():
        got = b.recv_report()[0].cpu().numpy()
        assert np.array_equal(got, _as_i32(m.report()[0]))
        return got
    for t in range(3):
        tick(t)
    got = check()
    assert (got[:, 6:15].sum(axis=1) > 0).all()
    b.recv_reset_streams([2, 5, 7], [9, 0, 3])
    m.reset_streams([2, 5, 7], [9, 0, 3])
    got = check()
    assert (got[[2, 5, 7], 6:15] == 0).all() and (got[[2, 5, 7], 15] == D).all() and (np.delete(got, [2, 5, 7], axis=0)[:, 6:15].sum(axis=1) > 0).all()
    stats = b.recv_stats()
    assert stats["inserted"] == m.stats[INSERTED] > 0                      # (the handle's statistics are not reset with the streams)
    b.recv_track(False)
    m.track(False)
    frozen = check()
    for t in range(3, 5):
        tick(t)
    got = check()
    assert np.array_equal(got[:, 6:], frozen[:, 6:]) and not np.array_equal(got[:, :6], frozen[:, :6])
    b.recv_track(True)
    m.track(True)
    assert (check()[:, 6:15] == 0).all()
    tick(5)
    assert check()[:, 6:15].sum() > 0
    b.recv_create(D, SLOT_SIM, 7)
    m.create(7)
    got = check()
    assert (got[:, 6:15] == 0).all() and (got[:, 15] == D).all() and (got[:, 0] == 7).all() and (got[:, 1:6] == 0).all()
    tick(7)                                                                # the switch is as it was: still counting
    assert check()[:, 6:15].sum() > 0
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("N,D", [(5, 1), (5, 4096), (4096, 8)])
def test_gpu_extremes_and_the_list_is_accepted_by_play_out(torch_cuda, N, D):
    """depth 1 and 4096 with a handful of streams, 4096 streams at the default depth with d_streams = NULL; two reports in a row with
    nothing between them give the same answer; the list a report produces is a list solo_recv_decode_streams accepts"""
    torch = torch_cuda
    b, payload, rows = _small_ring(torch, N, D, track=True)
    m = RingModel(N, D, SLOT_SIM)
    m.track(True)
    rng = np.random.default_rng(N + D)
    play0 = [int(v) for v in rng.integers(0, 3 * D + 5, N)] if N <= 64 else None
    if play0:
        b.recv_reset_streams(list(range(N)), play0)
        m.reset_streams(list(range(N)), play0)
    arr = []
    for s in range(N):
        p = m.play[s]
        offs = {0, D - 1, D // 2} if s % 4 == 0 else ({D - 1} if s % 4 == 1 else (set(int(v) for v in rng.integers(0, D, 6)) if s % 4 == 2 else set()))
        arr += [(s, p + k, int(rng.integers(0, 2))) for k in sorted(offs)]
        if s % 8 == 0:
            arr += [(s, p, 0), (s, p, 1), (s, p + D, 0)]
    _file(torch, b, m, payload, rows(arr))
    for min_ready, max_span in ((1, 0), (2, D), (0, 0), (D + 1, 0)):
        first = b.recv_report(min_ready=min_ready, max_span=max_span)
        second = b.recv_report(min_ready=min_ready, max_span=max_span)          # back to back, nothing in between
        w_rep, w_lst, w_rows = m.report(None, min_ready, max_span)
        for rep, lst, rws, cnt in (first, second):
            assert b.recv_report_count(cnt) == {"selected": len(w_lst), "listed": N}
            assert np.array_equal(rep.cpu().numpy(), _as_i32(w_rep))
            assert lst.cpu().numpy()[:len(w_lst)].tolist() == w_lst and rws.cpu().numpy()[:len(w_rows)].tolist() == w_rows
    rep, lst, rws, cnt = b.recv_report(min_ready=1, max_span=0)
    k = b.recv_report_count(cnt)["selected"]
    assert 0 < k < N
    pcm = torch.zeros((k, 1, b.packet_samples), dtype=torch.int16).cuda()
    st = torch.full((k,), -99, dtype=torch.int32).cuda()
    assert b.lib.solo_recv_decode_streams(b.h, lst.data_ptr(), k, 1, pcm.data_ptr(), st.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == 0).all()                                        # accepted (not -1); every packet is a valid one: decoded
    m.play_out(m.report(None, 1, 0)[1], 1)
    assert np.array_equal(b.recv_report()[0].cpu().numpy(), _as_i32(m.report()[0]))
    b.close()

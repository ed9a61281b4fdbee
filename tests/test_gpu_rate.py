"""solo_rate on the GPU: the controller (solo_amd.Rate) against tests/rate_model.py word for word at the workgroup edge; a running stream's
rate from device memory (SoloBatch.update_rates) against solo_batch_update_streams with the same values on a twin handle, against a handle
that was never updated, and against the poked compiled reference of tests/ref_ctl_poke.py; the ordering behind an encode in flight; the
list forms; the send mask against the model; the closed loop solo_rtcp_parse -> solo_rate_update -> solo_batch_update_rates ->
solo_batch_encode -> solo_rate_send_mask -> solo_send_pack captured in one graph and replayed against an eager twin; and thinning end
to end into a receiving handle's ring."""
import struct

import numpy as np
import pytest

import graph_replay_lib as G
import rate_model as M
import ref_ctl_poke as K
import refcodec as R
import solo_testlib as T

pytestmark = pytest.mark.gpu
need_ref = pytest.mark.skipif(not R.have_ref("fix"), reason="oracle/_ref not present on this box")

I32_MAX = 2 ** 31 - 1
# the knot lists of tests/test_gpu_update_streams.py, restated: TargetRate_table_NB[1..6] / _WB, and the rates that setup_rate clamps
KNOTS_NB = (8000, 9000, 11000, 13000, 16000, 22000)
KNOTS_WB = (11000, 14000, 17000, 21000, 26000, 36000)
LOW = (1, 6599, 6600)                                       # SILK rates 5000 (clamped up from -1599), 4999 (clamped), 5000
HIGH = (I32_MAX, 101601, 150000)                            # SILK rate clamped down to 100000
KEEP = (0, -5, -2 ** 31)
RATES_NB = list(dict.fromkeys(list(LOW) + [1600 + m * k + d for k in KNOTS_NB for m in (1, 2) for d in (-1, 0, 1)] + list(HIGH)))


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def words(blob):
    return np.ascontiguousarray(host(blob)).view(np.int32)


# ---- the controller ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows", [1, 255, 256, 257])
def test_controller_against_the_model(torch_cuda, n_rows):
    import solo_amd
    rc, m = solo_amd.Rate(n_rows), M.Rate(n_rows)
    p = M.TEST_PARAMS
    kw = {k: v for k, v in p.items() if k != "reserved"}
    assert np.array_equal(words(rc.get_state()), m.state())
    for c in range(M.CALLS):
        fb = M.feedback(n_rows, c)
        print("call", c)
        target, mode, count = rc.update(dev(fb), **kw)
        wt, wm, wc = m.update(fb, p)
        got = rc.count(count)
        print(got)
        assert got == wc, (c, got, wc)
        assert np.array_equal(host(target), wt) and np.array_equal(host(mode), wm), c
        assert np.array_equal(words(rc.get_state()), m.state()), c
        if c == 17 and n_rows > 2:                          # a listed reset in the middle of the run
            rows = list(range(1, n_rows, 3))
            rc.reset(rows)
            m.reset(rows)
        if c == 25:                                         # the state out and in again: all rows, then a list onto other rows
            blob = rc.get_state()
            rc.reset()
            assert np.array_equal(words(rc.get_state()), M.Rate(n_rows).state())
            rc.set_state(blob)
            assert np.array_equal(words(rc.get_state()), m.state())
            if n_rows > 4:
                src, dst = list(range(0, n_rows - 1, 2)), list(range(1, n_rows, 2))
                part = rc.get_state(src)
                assert np.array_equal(words(part), m.state(src))
                rc.set_state(part, dst)
                m.set_state(m.state(src), dst)
                assert np.array_equal(words(rc.get_state()), m.state())
    assert not M.REQUIRED_HITS - m.hits or n_rows < M.N_FAMILIES


def test_controller_refusals_and_binding_checks(torch_cuda):
    import solo_amd
    torch = torch_cuda
    rc = solo_amd.Rate(8)
    fb = dev(M.feedback(8, 0))
    before = words(rc.get_state())
    for bad in (dict(min_bps=6000, max_bps=40000, start_bps=5800), dict(min_bps=6000, max_bps=40000, start_bps=16000, quantum_bps=0),
                dict(min_bps=6100, max_bps=40000, start_bps=16000), dict(min_bps=6000, max_bps=40000, start_bps=16000, lo_q8=30),
                dict(min_bps=6000, max_bps=40000, start_bps=16000, thin_after=-1)):
        with pytest.raises(ValueError):
            rc.update(fb, **bad)
    ok = dict(min_bps=6000, max_bps=40000, start_bps=16000)
    for call in (lambda: rc.update(fb[:7], **ok), lambda: rc.update(fb.to(torch.int64), **ok), lambda: rc.update(fb.cpu(), **ok),
                 lambda: rc.update(fb, target=torch.zeros(7, dtype=torch.int32, device="cuda"), **ok),
                 lambda: rc.send_mask(torch.zeros(7, dtype=torch.uint8, device="cuda"), 1), lambda: rc.send_mask(torch.zeros(8, dtype=torch.uint8, device="cuda"), 0),
                 lambda: rc.send_mask(torch.zeros(8, dtype=torch.uint8, device="cuda"), 1, streams=[3, 1])):
        with pytest.raises(ValueError):
            call()
    prm = solo_amd.solo_rate_params_t(6000, 40000, 16000, 200, 5, 26, 13, 0, 250, 0, 3, 1)        # reserved != 0
    t, mo, cnt = (torch.zeros(16, dtype=torch.int32, device="cuda") for _ in range(3))
    import ctypes as C
    assert rc.lib.solo_rate_update(rc.h, fb.data_ptr(), C.byref(prm), t.data_ptr(), mo.data_ptr(), cnt.data_ptr(), rc._stream()) == -1
    prm.reserved = 0
    assert rc.lib.solo_rate_update(rc.h, fb.data_ptr() + 4, C.byref(prm), t.data_ptr(), mo.data_ptr(), cnt.data_ptr(), rc._stream()) == -1
    assert rc.lib.solo_rate_update(None, fb.data_ptr(), C.byref(prm), t.data_ptr(), mo.data_ptr(), cnt.data_ptr(), rc._stream()) == -1
    assert np.array_equal(words(rc.get_state()), before) and not host(cnt).any()


# ---- the send mask -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows,n_packets", [(1, 1), (7, 3), (256, 1), (257, 1), (300, 50), (3, 257)])
def test_send_mask_against_the_model(torch_cuda, n_rows, n_packets):
    import solo_amd
    torch = torch_cuda
    rng = np.random.default_rng(n_rows * 1000 + n_packets)
    rc = solo_amd.Rate(n_rows)
    mode = rng.integers(0, 2, n_rows).astype(np.uint8)
    base = rng.integers(-2 ** 31, 2 ** 31, n_rows).astype(np.int32)
    sin = rng.integers(0, 4, (n_rows, n_packets)).astype(np.uint8)
    for first in (0, 7, -3):
        assert np.array_equal(host(rc.send_mask(dev(mode), n_packets, first_seq=first)), M.send_mask(mode, n_packets, first_seq=first))
        want = M.send_mask(mode, n_packets, seq_base=base, first_seq=first, send_in=sin)
        assert np.array_equal(host(rc.send_mask(dev(mode), n_packets, seq_base=dev(base), first_seq=first, send=dev(sin))), want)
        buf = dev(sin)
        assert rc.send_mask(dev(mode), n_packets, seq_base=dev(base), first_seq=first, send=buf, out=buf) is buf and np.array_equal(host(buf), want)
    if n_rows > 2:
        lst = sorted(rng.choice(n_rows, size=max(2, n_rows // 3), replace=False).tolist())
        want = M.send_mask(mode, n_packets, streams=lst, seq_base=base[:len(lst)], first_seq=11, send_in=sin[:len(lst)])
        got = rc.send_mask(dev(mode), n_packets, streams=lst, seq_base=dev(base[:len(lst)]), first_seq=11, send=dev(sin[:len(lst)]))
        assert np.array_equal(host(got), want)
        bad = np.array(lst, np.int32)
        bad[[0, -1]] = bad[[-1, 0]]                         # not increasing: nothing is written, in any workgroup
        out = torch.full((len(lst), n_packets), 0xEE, dtype=torch.uint8, device="cuda")
        rc.send_mask(dev(mode), n_packets, streams=dev(bad), first_seq=11, out=out)
        assert (host(out) == 0xEE).all()
        bad = np.array(lst, np.int32)
        bad[-1] = n_rows                                    # outside the object
        rc.send_mask(dev(mode), n_packets, streams=dev(bad), first_seq=11, out=out)
        assert (host(out) == 0xEE).all()


# ---- a running stream's rate from device memory --------------------------------------------------------------------------------------------
def _pcm(N, P, samples, seed):
    sig = [T.synth_stream_32k(seed + i, P) if samples == 1280 else R.synth_stream(seed + i, P) for i in range(min(N, 8))]
    return np.stack([sig[i % len(sig)] for i in range(N)])


def _encode(b, x):
    bits, nb, st = b.encode(dev(x))
    return bits, nb, st


def _enc_state(b, N):
    blob, cnt = b.export_streams(list(range(N)), which="enc")
    assert b.migrate_count(cnt)["streams"] == N
    return host(blob)


def _three_handles(torch, kw, N, calls, values, wb=False, joint=False, seed=400):
    """values[c]: int32 [N], what update_rates takes before call c (None: no call).  -> nothing; asserts the three comparisons"""
    import solo_amd
    samples = 1280 if wb else 640
    P = sum(calls)
    pcm = _pcm(N, P, samples, seed)
    hs = {k: solo_amd.SoloBatch(N, encoder=True, decoder=False, slot_bytes=1024, **kw) for k in ("device", "host", "never")}
    ctl = [((i // 2) % 2, (i // 3) % 2) for i in range(N)]                  # every stream's own DTX / useMDIndex, set before the run
    for b in hs.values():
        b.reset_streams(range(N), dtx=[c[0] for c in ctl], use_md_index=[c[1] for c in ctl], which="enc")
    out = {k: [] for k in hs}
    p0 = 0
    touched = set()
    for c, n_p in enumerate(calls):
        v = values[c]
        if v is not None:
            kinds = [M.apply_target(int(x), joint, wb)[0] for x in v]
            cnt = hs["device"].update_rates(dev(np.asarray(v, np.int32)))
            got = hs["device"].rates_count(cnt)
            want = dict(applied=kinds.count("applied"), kept=kinds.count("kept"), refused=kinds.count("refused"), listed=N)
            print("call", c, got)
            assert got == want, (c, got, want)
            upd = [i for i in range(N) if kinds[i] == "applied"]
            touched |= set(upd)
            if upd:
                hs["host"].update_streams(upd, rate=[int(v[i]) for i in upd], dtx=[ctl[i][0] for i in upd], use_md_index=[ctl[i][1] for i in upd], which="enc")
        for k, b in hs.items():
            bits, nb, st = _encode(b, pcm[:, p0:p0 + n_p])
            out[k].append((host(bits), host(nb), host(st)))
        p0 += n_p
    cat = {k: [np.concatenate([o[j] for o in out[k]], axis=1) if j < 2 else np.stack([o[j] for o in out[k]]) for j in range(3)] for k in hs}
    for k in hs:
        assert not cat[k][2].any(), k
    assert np.array_equal(cat["device"][1], cat["host"][1]), "d_nbytes: device call against host call"
    assert np.array_equal(cat["device"][0], cat["host"][0]), "payload bytes: device call against host call"
    kept = [i for i in range(N) if i not in touched]
    assert kept and touched
    assert np.array_equal(cat["device"][0][kept], cat["never"][0][kept]) and np.array_equal(cat["device"][1][kept], cat["never"][1][kept])
    moved = sorted(touched)
    assert not np.array_equal(cat["device"][0][moved], cat["never"][0][moved])
    sd, sh, sn = (_enc_state(hs[k], N) for k in ("device", "host", "never"))
    assert np.array_equal(sd, sh), "exported encoder states: device call against host call"
    assert np.array_equal(sd[kept], sn[kept])
    for b in hs.values():
        b.close()


def test_update_rates_against_update_streams(torch_cuda):
    N = 257
    rates = RATES_NB
    nth = lambda i, m: i - i // 4 - (m > 1) * ((i + 2) // 4)                 # how many positions in front of i take a rate
    v1 = [KEEP[i % 3] if i % 4 == 0 else rates[nth(i, 1) % len(rates)] for i in range(N)]
    v2 = [KEEP[i % 3] if i % 4 in (0, 1) else rates[(nth(i, 2) + 17) % len(rates)] for i in range(N)]
    assert set(rates) <= set(v1) | set(v2) and set(KEEP) <= set(v1)
    _three_handles(torch_cuda, {}, N, (2, 1, 2), [None, v1, v2])


def test_update_rates_32k_refuses_below_the_floor(torch_cuda):
    v1 = [15599, 1, 15600, 24000, 0, 14000]                 # SILK 13999, < 0, 14000, 22400, keep, 12400
    v2 = [I32_MAX, 14000, 0, 15599, 0, 1600 + 2 * 21000 + 1]   # stream 1 is refused twice, stream 4 kept twice: the never-updated twin's
    kinds = [M.apply_target(x, False, True)[0] for x in v1 + v2]
    assert kinds.count("refused") == 5 and kinds.count("kept") == 3
    _three_handles(torch_cuda, dict(samplerate=32000, rate=15600), 6, (2, 1, 2), [None, v1, v2], wb=True)


def test_update_rates_joint_mode_takes_800(torch_cuda):
    v1 = [801, 800 + 9000, 0, 800 + 2 * 13000 - 1, 13600, I32_MAX]
    v2 = [0, 800 + 8000 + 1, 0, 5800, 100801, 0]
    _three_handles(torch_cuda, dict(joint=1), 6, (2, 1, 2), [None, v1, v2], joint=True)


@need_ref
def test_update_rates_against_the_compiled_reference(torch_cuda):
    import solo_amd
    N, calls = 6, (2, 2, 2)
    P = sum(calls)
    pcm = np.stack([R.synth_stream(430 + i, P) for i in range(N)])
    vals = [None, [24000, 0, 6599, 1600 + 2 * 11000 + 1, -1, I32_MAX], [0, 9600, 13600, 0, 1600 + 8000 - 1, 40000]]
    b = solo_amd.SoloBatch(N, encoder=True, decoder=False, slot_bytes=1024)
    got, p0 = [], 0
    for c, n_p in enumerate(calls):
        if vals[c] is not None:
            b.update_rates(dev(np.array(vals[c], np.int32)))
        bits, nb, st = _encode(b, pcm[:, p0:p0 + n_p])
        got.append((host(bits), host(nb)))
        assert not host(st).any()
        p0 += n_p
    hb, hn = np.concatenate([g[0] for g in got], 1), np.concatenate([g[1] for g in got], 1)
    for i in range(N):
        e = K.PokeEncoder("fix")
        p = 0
        for c, n_p in enumerate(calls):
            if vals[c] is not None and vals[c][i] > 0:
                e.set_control(rate=vals[c][i], dtx=0, use_md_index=0)
            for _ in range(n_p):
                pl, n0, n1 = e.encode(pcm[i, p])
                assert (int(hn[i, p, 0]), int(hn[i, p, 1])) == (n0, n1) and hb[i, p, :n0].tobytes() == pl[:n0], (i, p)
                p += 1


def test_update_rates_ordering_without_host_waits(torch_cuda):
    """an encode of 3 packets, the update, an encode of 2 packets, nothing in between: the first call's packets keep the old rate"""
    import solo_amd
    torch = torch_cuda
    N = 64
    pcm = _pcm(N, 5, 640, 440)
    v = np.array([RATES_NB[(3 * i) % len(RATES_NB)] if i % 3 else 0 for i in range(N)], np.int32)
    outs = []
    for waits in (False, True):
        b = solo_amd.SoloBatch(N, encoder=True, decoder=False, slot_bytes=1024)
        x1, x2, dv = dev(pcm[:, :3]), dev(pcm[:, 3:]), dev(v)
        torch.cuda.synchronize()
        b1 = b.encode(x1)
        if waits:
            torch.cuda.synchronize()
        cnt = b.update_rates(dv)
        if waits:
            torch.cuda.synchronize()
        b2 = b.encode(x2)
        torch.cuda.synchronize()
        assert b.rates_count(cnt)["applied"] == int((v > 0).sum())
        outs.append([host(t) for t in b1[:2] + b2[:2]] + [_enc_state(b, N)])
        b.close()
    for x, y in zip(*outs):
        assert np.array_equal(x, y)


def test_update_rates_list_forms(torch_cuda):
    import solo_amd
    torch = torch_cuda
    N = 40
    pcm = _pcm(N, 2, 640, 450)
    lst = [1, 2, 5, 17, 39]
    v = np.array([24000, 0, 9000, I32_MAX, 6600], np.int32)
    full = np.zeros(N, np.int32)
    full[lst] = v
    a, b = (solo_amd.SoloBatch(N, encoder=True, decoder=False, slot_bytes=1024) for _ in range(2))
    ca = a.update_rates(dev(v), streams=lst)
    cb = b.update_rates(dev(full))
    assert a.rates_count(ca) == dict(applied=4, kept=1, refused=0, listed=5) and b.rates_count(cb) == dict(applied=4, kept=N - 4, refused=0, listed=N)
    ra, rb = _encode(a, pcm), _encode(b, pcm)
    assert np.array_equal(host(ra[0]), host(rb[0])) and np.array_equal(host(ra[1]), host(rb[1]))
    before = _enc_state(a, N)
    assert np.array_equal(before, _enc_state(b, N))
    for bad in ([2, 1, 5, 17, 39], [1, 2, 5, 17, N], [1, 1, 5, 17, 39], [-1, 2, 5, 17, 39]):
        cnt = torch.full((4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        r = a.lib.solo_batch_update_rates(a.h, dev(np.array(bad, np.int32)).data_ptr(), 5, dev(v).data_ptr(), cnt.data_ptr(), a._stream())
        assert r == 0 and int(host(cnt)[0]) == -1, bad
        assert np.array_equal(_enc_state(a, N), before), bad
    # the host's refusals, and a handle without an encoder
    cnt, dv, dl = torch.zeros(4, dtype=torch.int32, device="cuda"), dev(v), dev(np.array(lst, np.int32))
    f = a.lib.solo_batch_update_rates
    assert f(a.h, dl.data_ptr(), 0, dv.data_ptr(), cnt.data_ptr(), a._stream()) == -1 and f(a.h, dl.data_ptr(), N + 1, dv.data_ptr(), cnt.data_ptr(), a._stream()) == -1
    assert f(a.h, None, 5, dv.data_ptr(), cnt.data_ptr(), a._stream()) == -1 and f(a.h, dl.data_ptr(), 5, None, cnt.data_ptr(), a._stream()) == -1
    assert f(a.h, dl.data_ptr(), 5, dv.data_ptr(), None, a._stream()) == -1 and f(None, dl.data_ptr(), 5, dv.data_ptr(), cnt.data_ptr(), a._stream()) == -1
    assert f(a.h, dl.data_ptr() + 2, 4, dv.data_ptr(), cnt.data_ptr(), a._stream()) == -1
    d = solo_amd.SoloBatch(4, encoder=False, decoder=True)
    assert f(d.h, None, 4, dv.data_ptr(), cnt.data_ptr(), d._stream()) == -1
    with pytest.raises(ValueError):
        d.update_rates(dv[:4])
    for call in (lambda: a.update_rates(dv), lambda: a.update_rates(dv, streams=[2, 1, 5, 17, 39]), lambda: a.update_rates(dv.to(torch.int64), streams=lst),
                 lambda: a.update_rates(v, streams=lst)):
        with pytest.raises(ValueError):
            call()
    assert np.array_equal(_enc_state(a, N), before) and not host(cnt).any()


# ---- the closed loop under capture ---------------------------------------------------------------------------------------------------------
def _rr(sender, ours, fraction, cum, ehs, lsr, dlsr):
    """a receiver report with one block"""
    return struct.pack(">BBHI", 0x81, 201, 7, sender) + struct.pack(">IIIIII", ours, (fraction << 24) | (cum & 0xFFFFFF), ehs, 5, lsr, dlsr)


def _bye(sender):
    """an empty receiver report (a compound packet begins with a report) and a BYE of the same source"""
    return struct.pack(">BBHI", 0x80, 201, 1, sender) + struct.pack(">BBHI", 0x81, 203, 1, sender)


LOOP_PARAMS = M.params(6000, 40000, 13600, thin_after=1, thin_release=2)


def test_capture_closed_loop(torch_cuda):
    """the sender's RTCP tick in ONE graph, 8 streams: replay k parses other reports, so other streams change their rate and their mode,
    encodes another packet and packs it under the mask; everything equals the same calls issued eagerly on a twin, and the controller
    equals the model fed with the feedback the graph itself produced"""
    G.need_four_queues()
    import ctypes as C
    import solo_amd
    import test_gpu_rtcp as TR
    torch = torch_cuda
    n, D, W, SLOT, NOW = 8, 16, 1024, 512, (0x83AA7E80 << 32)
    X, Y = TR.sessions(n)                                   # X: the peers' sources (r_rx), Y: ours (r_tx)
    rx, ry = TR.gpu_session(X), TR.gpu_session(Y)
    z = G.fixture()
    feeds = []
    for k in range(6):
        now = NOW + (k << 32)
        mid = (now >> 16) & 0xFFFFFFFF
        dgs = []
        for s in range(n):
            fraction = (255, 0, 10, (0, 40)[k % 2], None, 0, 0, 3)[s]
            if fraction is None or (s == 6 and k % 2):
                continue                                    # stream 4 never hears from its peer, stream 6 every other tick
            if s == 5 and k == 3:
                dgs.append(_bye(X.ssrc[s]))
                continue
            dgs.append(_rr(X.ssrc[s], Y.ssrc[s], fraction, 3 * k, 1000 + 50 * k + s, (mid - 0x3000) & 0xFFFFFFFF, 0x1000 + 16 * s))
        table, wire, at = np.zeros((D, 2), np.int32), np.zeros(W, np.uint8), 3 * k
        for i, d in enumerate(dgs):
            table[i] = (at, len(d))
            wire[at:at + len(d)] = np.frombuffer(d, np.uint8)
            at += len(d) + (k + i) % 3
        feeds.append(dict(dgrams=table, wire=wire, now=np.array([now], np.uint64).view(np.int64), pcm=z["pcm"][:, k:k + 1],
                          seq_base=np.array([100 * k + 3 * s for s in range(n)], np.int32)))
    prm = solo_amd.solo_rate_params_t(*[int(v) for v in M.params_words(LOOP_PARAMS)])

    def make():
        tx = solo_amd.SoloBatch(n, encoder=True, decoder=False, slot_bytes=SLOT)
        rtcp, rate = solo_amd.Rtcp(n), solo_amd.Rate(n)
        i32, u8 = torch.int32, torch.uint8
        ins = dict(dgrams=G.zeros(torch, (D, 2), i32), wire=G.zeros(torch, (W,), u8), now=G.zeros(torch, (1,), torch.int64),
                   pcm=G.zeros(torch, (n, 1, 640), torch.int16), seq_base=G.zeros(torch, (n,), i32))
        outs = dict(feedback=G.zeros(torch, (n, 8), i32), pcount=G.zeros(torch, (16,), i32), target=G.zeros(torch, (n,), i32), mode=G.zeros(torch, (n,), u8),
                    rcount=G.zeros(torch, (16,), i32), acount=G.zeros(torch, (4,), i32), bits=G.zeros(torch, (n, 1, SLOT), u8),
                    nbytes=G.zeros(torch, (n, 1, 2), torch.int16), status=G.zeros(torch, (n,), i32), send=G.zeros(torch, (n, 1), u8),
                    records=G.zeros(torch, (2 * n, 5), i32), payload=G.zeros(torch, (n * SLOT,), u8), scount=G.zeros(torch, (8,), i32))
        p = lambda name: (ins[name] if name in ins else outs[name]).data_ptr()

        def call():
            st = tx._stream()
            return [rtcp.lib.solo_rtcp_parse(rtcp.h, rx.h, ry.h, p("dgrams"), D, p("wire"), W, 0, p("now"), p("feedback"), p("pcount"), st),
                    rate.lib.solo_rate_update(rate.h, p("feedback"), C.byref(prm), p("target"), p("mode"), p("rcount"), st),
                    tx.lib.solo_batch_update_rates(tx.h, None, n, p("target"), p("acount"), st),
                    tx.lib.solo_batch_encode(tx.h, p("pcm"), 1, p("bits"), p("nbytes"), p("status"), st),
                    rate.lib.solo_rate_send_mask(p("mode"), n, None, n, 1, p("seq_base"), 500, None, p("send"), st),
                    tx.lib.solo_send_pack(tx.h, p("bits"), p("nbytes"), p("send"), 1, p("seq_base"), 500, p("records"), 2 * n, p("payload"), n * SLOT,
                                          p("scount"), st)]

        def run():
            r = call()
            return 0 if not any(r) else r

        def state():
            return np.concatenate([words(rate.get_state()).ravel(), np.ascontiguousarray(host(rtcp.get_state())).view(np.int32).ravel()])
        return G.Stage(torch, ins, outs, run, state=state, keep=(tx, rtcp, rate))

    mdl = M.Rate(n)
    seen_modes, rates = set(), set()

    def model(k, feed, got):
        wt, wm, wc = mdl.update(got["feedback"], LOOP_PARAMS)
        assert np.array_equal(got["target"], wt) and np.array_equal(got["mode"], wm), (k, got["target"], wt)
        assert dict(zip(M.COUNT, (int(v) for v in got["rcount"]))) == wc and not got["rcount"][len(M.COUNT):].any(), k
        assert got["acount"].tolist() == [int((wt > 0).sum()), int((wt <= 0).sum()), 0, n] and not got["status"].any(), k
        want = M.send_mask(wm, 1, seq_base=feed["seq_base"], first_seq=500)
        assert np.array_equal(got["send"], want)
        nrec = int(got["scount"][0])
        assert nrec == int(sum(bin(int(v)).count("1") for v in want[:, 0])) and int(got["pcount"][6]) > 0
        seen_modes.add(tuple(wm.tolist()))
        rates.update(int(v) for v in wt)

    _, cap, twin = G.replay_against_twin(torch, make, feeds, model=model, stateful=True)
    assert np.array_equal(cap.state()[:n * M.WORDS].reshape(n, M.WORDS), mdl.state())
    assert len(seen_modes) > 1 and len(rates) > 3 and any(m[0] for m in seen_modes)
    assert np.array_equal(_enc_state(cap.keep[0], n), _enc_state(twin.keep[0], n))


# ---- thinning end to end --------------------------------------------------------------------------------------------------------------------
def test_thinning_end_to_end(torch_cuda):
    """a thin stream leaves solo_send_pack as exactly one datagram per non-empty packet, MD1 on even and MD2 || HB on odd sequence
    numbers, and a receiving handle's ring plays it out from single descriptions with status 0 -- as a decoder does that is given the mask"""
    import solo_amd
    torch = torch_cuda
    N, P, FIRST = 6, 8, 1001
    pcm = _pcm(N, P, 640, 460)
    tx = solo_amd.SoloBatch(N, encoder=True, decoder=False)
    bits, nb, st = tx.encode(dev(pcm))
    rc = solo_amd.Rate(N)
    mode = np.array([1, 0, 1, 1, 0, 1], np.uint8)
    base = np.array([0, 5, 1, 10, 3, 7], np.int32)
    mask = rc.send_mask(dev(mode), P, seq_base=dev(base), first_seq=FIRST)
    rec, pay, cnt = tx.send_pack(bits, nb, send=mask, first_seq=FIRST, seq_base=dev(base))
    c = tx.send_count(cnt)
    hrec, hn = host(rec)[:c["records"]], host(nb)
    assert not host(st).any() and c["refused"] == 0 and c["empty"] == 0 and c["records"] == c["records_needed"]
    for i in range(N):
        mine = hrec[hrec[:, 0] == i]
        if not mode[i]:
            assert len(mine) == 2 * P
            continue
        assert len(mine) == P and sorted(mine[:, 1].tolist()) == [FIRST + int(base[i]) + p for p in range(P)], i
        assert all(int(r[2]) == (int(r[1]) & 1) for r in mine), i
        assert {int(r[2]) for r in mine} == {0, 1}
    assert c["records"] == int((mode == 0).sum()) * 2 * P + int((mode == 1).sum()) * P
    rx = solo_amd.SoloBatch(N, encoder=False, decoder=True)
    rx.recv_create(P, 256, 0)
    rx.recv_reset_streams(list(range(N)), [FIRST + int(v) for v in base])
    rx.recv_insert(rec.contiguous(), pay)
    stats = rx.recv_stats()
    assert stats["inserted"] == c["records"] and stats["late"] == stats["ahead"] == stats["duplicate"] == 0, stats
    got, st2 = rx.recv_decode(P)
    want_dec = solo_amd.SoloBatch(N, encoder=False, decoder=True)
    want, st3 = want_dec.decode(bits, nb, mask)
    assert not host(st2).any() and not host(st3).any()
    assert np.array_equal(host(got), host(want))
    assert all(np.abs(host(got)[i].astype(np.int32)).max() > 100 for i in range(N))

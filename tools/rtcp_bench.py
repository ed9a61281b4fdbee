#!/usr/bin/env python3
"""Cost of the RTCP calls (solo_rtcp_received, solo_rtcp_sent, solo_rtcp_build, solo_rtcp_parse) at 4096 streams x 1 packet (a tick of
8192 datagrams) and x 50, 13.6 kbps, next to their neighbours in the tick on the same data, in one run:

  (a) solo_rtcp_received of the arrivals solo_rtp_parse wrote, with d_arrival_time and with the scalar; and the ADVERSARIAL call in
      which one stream owns every datagram of the tick (the arrivals' stream column overwritten)
  (b) solo_rtcp_sent of the records and datagrams solo_rtp_pack left
  (c) solo_rtcp_build of one report per stream (SR + report block + SDES: every stream has sent and received; a solo_rtcp_sent in front
      of every call keeps them SRs, timed alone and taken off) and solo_rtcp_parse of those reports by the peer
  (d) solo_rtp_pack, solo_rtp_parse and solo_recv_insert, the neighbours (the ring is emptied before every insert; that reset is timed
      alone and taken off)

Every call goes through the C ABI with buffers allocated once.  Every figure is ms per call: HIP events around `iters` back-to-back
calls, `iters` chosen per stage so that a window lasts about 50 ms, after a warm-up of the same calls; the median over `runs` windows,
with the smallest and the largest next to it.  Back-to-back calls measure the larger of the host's enqueue time and the device's time
per call: the figures BOUND THE CALL FROM ABOVE and are not kernel time -- solo_rtcp_received is eight short launches, and at a
one-packet tick the host's share may be all of it.  Read (a) - (c) against (d), measured the same way.  The statistics keep running
while the same arrivals are filed again and again: from the second call on a stream sees its sequence numbers repeat, which changes the
branch update_seq takes and not the work.

  python tools/rtcp_bench.py [--streams 4096] [--packets 1 50] [--runs 9] [--out profiles/rtcp.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import solo_amd                       # noqa: E402
from solo_amd.synth import synth_stream  # noqa: E402
from rtp_bench import timed           # noqa: E402


def minus(a, b):
    """the figures of a pair of calls without the first of the pair"""
    out = dict(a)
    for k in ("ms", "min_ms", "max_ms"):
        out[k] = round(a[k] - b["ms"], 5)
    return out


def shape(torch, N, P, runs):
    pcm = torch.from_numpy(np.stack([synth_stream(i % 64, P) for i in range(N)]).reshape(N, P, 640)).cuda()
    tx = solo_amd.SoloBatch(N, rate=13600, encoder=True, decoder=False, slot_bytes=512)
    bits, nb, _ = tx.encode(pcm)
    records, payload, scount = tx.send_pack(bits, nb, first_seq=1000)
    sc = tx.send_count(scount)
    assert sc["records"] == sc["records_needed"] and sc["refused"] == 0
    n, M = sc["records"], records.shape[0]
    rng = np.random.default_rng(1)
    ours, theirs = solo_amd.Rtp(N, 640), solo_amd.Rtp(N, 640)
    for r, mul in ((ours, 2654435761), (theirs, 2246822519)):
        r.bind(list(range(N)), [(i + 1) * mul % 2 ** 32 for i in range(N)], [int(v) for v in rng.integers(0, 2 ** 32, N)],
               [int(v) for v in rng.integers(0, 2 ** 16, N)], (96, 97))
    st, L = tx._stream(), tx.lib
    res = {"streams": N, "packets": P, "datagrams": n}
    z = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device="cuda")
    cap = sc["bytes"] + 23 * M
    # (d) pack, parse, insert
    dgrams, wire, cnt = z((M, 2), torch.int32), z((cap,), torch.uint8), z((8,), torch.int32)
    res["d_rtp_pack"] = timed(torch, lambda: L.solo_rtp_pack(ours.h, records.data_ptr(), scount.data_ptr(), M, payload.data_ptr(), payload.shape[0], None, 0,
                                                             dgrams.data_ptr(), wire.data_ptr(), cap, cnt.data_ptr(), st), runs)
    assert ours.pack_count(cnt)["dgrams"] == n
    rx = solo_amd.SoloBatch(N, encoder=False, decoder=True)
    depth = 64
    rx.recv_create(depth, 256, 1000)
    arrivals, sq_out, pcnt = z((n, 5), torch.int32), z((n,), torch.int16), z((8,), torch.int32)
    res["d_rtp_parse"] = timed(torch, lambda: L.solo_rtp_parse(ours.h, rx.h, dgrams.data_ptr(), n, wire.data_ptr(), wire.shape[0], arrivals.data_ptr(), None,
                                                               sq_out.data_ptr(), pcnt.data_ptr(), st), runs)
    assert ours.parse_count(pcnt)["accepted"] == n

    def reset():
        return L.solo_recv_create(rx.h, depth, 256, 1000, st)
    rst = timed(torch, reset, runs)
    res["d_recv_insert"] = minus(timed(torch, lambda: reset() or L.solo_recv_insert(rx.h, arrivals.data_ptr(), n, wire.data_ptr(), wire.shape[0], st), runs), rst)
    res["d_recv_insert"]["ring_reset_ms"] = rst["ms"]
    assert rx.recv_stats()["inserted"] == n
    # (a) received: we hear the streams `ours` describes (the loop of this bench: what we packed is what we parse)
    rtcp, peer = solo_amd.Rtcp(N), solo_amd.Rtcp(N)
    for o in (rtcp, peer):
        o.set_cname(range(N), ["stream%d@bench.example" % i for i in range(N)])
    atime = torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32)).cuda()
    rcnt = z((8,), torch.int32)

    def received(arr, at):
        return lambda: L.solo_rtcp_received(rtcp.h, ours.h, arr.data_ptr(), sq_out.data_ptr(), n, None if at is None else at.data_ptr(), 12345, rcnt.data_ptr(), st)
    res["a_received_times"] = timed(torch, received(arrivals, atime), runs)
    c = rtcp.count("received", rcnt)
    assert c["counted"] == n and c["not_counted"] == 0, c
    res["a_received_scalar"] = timed(torch, received(arrivals, None), runs)
    if P == 1:                          # the adversarial tick: one stream owns all of it
        one = arrivals.clone()
        one[:, 0] = 7
        res["a_received_one_stream"] = timed(torch, received(one, atime), runs)
        c = rtcp.count("received", rcnt)
        assert c["counted"] == n, c
        res["a_received_one_stream"]["last_call"] = c
    # (b) sent
    tcnt = z((8,), torch.int32)

    def sent():
        return L.solo_rtcp_sent(rtcp.h, ours.h, records.data_ptr(), scount.data_ptr(), M, dgrams.data_ptr(), tcnt.data_ptr(), st)
    res["b_sent"] = timed(torch, sent, runs)
    assert rtcp.count("sent", tcnt)["sent"] == n
    # (c) build: one report per stream -- we send as `theirs` and hear `ours` --, parsed by the peer, who sends as `ours` and hears `theirs`
    idx = torch.arange(N, dtype=torch.int32, device="cuda")
    rd, rw, bcnt = z((N, 2), torch.int32), z((96 * N,), torch.uint8), z((8,), torch.int32)
    now = (0x83AA7E80 << 32) | 0x1234

    def build():
        return sent() or L.solo_rtcp_build(rtcp.h, theirs.h, ours.h, idx.data_ptr(), N, now, None, rd.data_ptr(), rw.data_ptr(), 96 * N, bcnt.data_ptr(), st)
    res["c_build"] = minus(timed(torch, build, runs), res["b_sent"])
    bc = rtcp.count("build", bcnt)
    assert bc["built"] == N and bc["with_sr"] == N and bc["refused"] == 0, bc
    res["c_build"]["bytes"] = bc["bytes"]
    fb, qcnt = z((N, 8), torch.int32), z((16,), torch.int32)
    res["c_parse"] = timed(torch, lambda: L.solo_rtcp_parse(peer.h, theirs.h, ours.h, rd.data_ptr(), N, rw.data_ptr(), 96 * N, now + (1 << 32), None, fb.data_ptr(),
                                                            qcnt.data_ptr(), st), runs)
    pc = peer.count("parse", qcnt)
    assert pc["accepted"] == N and pc["sr"] == N and pc["blocks"] == N, pc
    res["ratios"] = {"received_times_over_recv_insert": round(res["a_received_times"]["ms"] / res["d_recv_insert"]["ms"], 3),
                     "received_scalar_over_recv_insert": round(res["a_received_scalar"]["ms"] / res["d_recv_insert"]["ms"], 3),
                     "received_times_over_rtp_parse": round(res["a_received_times"]["ms"] / res["d_rtp_parse"]["ms"], 3),
                     "sent_over_rtp_pack": round(res["b_sent"]["ms"] / res["d_rtp_pack"]["ms"], 3)}
    if P == 1:
        res["ratios"]["one_stream_over_normal"] = round(res["a_received_one_stream"]["ms"] / res["a_received_times"]["ms"], 3)
    for o in (rtcp, peer, ours, theirs, tx, rx):
        o.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--packets", type=int, nargs="+", default=[1, 50])
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    res = {"runs": a.runs, "kernel_source_hash": solo_amd.kernel_source_hash(), "shader_clock_mhz_before": solo_amd.shader_clock_mhz(), "shapes": []}
    for P in a.packets:
        res["shapes"].append(shape(torch, a.streams, P, a.runs))
    res["shader_clock_mhz_after"] = solo_amd.shader_clock_mhz()
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()

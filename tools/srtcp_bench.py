#!/usr/bin/env python3
"""Cost of the SRTCP calls (solo_srtcp_protect, solo_srtcp_unprotect) at 4096 streams, one report per stream (SR + report block + SDES),
next to the calls they stand around, in one run:

  (a) solo_rtcp_build of 4096 packets alone, without and with the 14-byte trailer (a solo_rtcp_sent in front of every call keeps them
      SRs; it is timed alone and taken off, as in tools/rtcp_bench.py)
  (b) solo_rtcp_build with the trailer + solo_srtcp_protect, and from that solo_srtcp_protect alone
  (c) solo_rtcp_parse of the reports in the clear, alone
  (d) solo_srtcp_unprotect + solo_rtcp_parse of the protected reports, and from that solo_srtcp_unprotect alone.  A datagram is accepted
      only once, so the bench protects 64 batches with rising indices and a window is exactly one walk through them, the receive
      records set back to "none yet" in front of it: every datagram is accepted and pays its MAC and its cipher.  The same walk with the
      records left at the last batch (everything `replayed`: no MAC, no cipher) is timed beside it.  unprotect works in place, so a call
      copies its batch first; the copy is timed alone and taken off

Every call goes through the C ABI with buffers allocated once.  Every figure is ms per call as in tools/rtp_bench.py (HIP events around
back-to-back calls, windows of about 50 ms, the median over `runs` windows with the smallest and the largest): the figures BOUND THE CALL
FROM ABOVE and are not kernel time.  Bytes per packet are reported beside them.

  python tools/srtcp_bench.py [--streams 4096] [--runs 9] [--out profiles/srtcp.json] [--rtcp-before FILE --rtcp-after FILE]

--rtcp-before / --rtcp-after: results of tools/rtcp_bench.py on the parent commit and on this one; their c_build figures are recorded
(a trailer of 0 must leave solo_rtcp_build where it was).
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
from rtp_bench import timed           # noqa: E402
from rtcp_bench import minus          # noqa: E402

BATCHES = 64                          # protected batches the unprotect calls of a window walk through, each newer than the one before


def run(torch, N, runs):
    rng = np.random.default_rng(1)
    ours, theirs = solo_amd.Rtp(N, 640), solo_amd.Rtp(N, 640)
    for r, mul in ((ours, 2654435761), (theirs, 2246822519)):
        r.bind(list(range(N)), [(i + 1) * mul % 2 ** 32 for i in range(N)], [int(v) for v in rng.integers(0, 2 ** 32, N)],
               [int(v) for v in rng.integers(0, 2 ** 16, N)], (96, 97))
    master = [rng.integers(0, 256, 30, dtype=np.uint8).tobytes() for _ in range(N)]
    theirs.set_rtcp_keys(range(N), tx=master, rx=master)                  # we send as `theirs`; the peer hears `theirs` with the same keys
    st, L = ours._stream(), ours.lib
    z = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device="cuda")
    rtcp, peer = solo_amd.Rtcp(N), solo_amd.Rtcp(N)
    rtcp.set_cname(range(N), ["stream%d@bench.example" % i for i in range(N)])
    # every stream has received (a report block) and sends (an SR)
    arr = np.zeros((N, 5), np.int32)
    arr[:, 0], arr[:, 1], arr[:, 4] = np.arange(N), 10, 40
    rcnt = rtcp.received(ours, torch.from_numpy(arr).cuda(), z((N,), torch.int16), None, 12345)
    assert rtcp.count("received", rcnt)["counted"] == N
    records, scount, dg1 = torch.from_numpy(arr).cuda(), torch.tensor([N, N, 0, 0, 0, 0, 0, 0], dtype=torch.int32, device="cuda"), z((N, 2), torch.int32)
    dg1[:, 1] = 52
    tcnt = z((8,), torch.int32)

    def sent():
        return L.solo_rtcp_sent(rtcp.h, theirs.h, records.data_ptr(), scount.data_ptr(), N, dg1.data_ptr(), tcnt.data_ptr(), st)
    res = {"streams": N, "sent_in_front": timed(torch, sent, runs)}
    idx = torch.arange(N, dtype=torch.int32, device="cuda")
    CAP = 112 * N
    rd, rw, bcnt, scnt = z((N, 2), torch.int32), z((CAP,), torch.uint8), z((8,), torch.int32), z((8,), torch.int32)
    now = (0x83AA7E80 << 32) | 0x1234

    def build():
        return sent() or L.solo_rtcp_build(rtcp.h, theirs.h, ours.h, idx.data_ptr(), N, now, None, rd.data_ptr(), rw.data_ptr(), CAP, bcnt.data_ptr(), st)

    def build_protect():
        return build() or L.solo_srtcp_protect(rtcp.h, theirs.h, idx.data_ptr(), N, bcnt.data_ptr(), rd.data_ptr(), rw.data_ptr(), CAP, scnt.data_ptr(), st)
    # (a) build alone, trailer 0 and 14
    res["a_build_trailer_0"] = minus(timed(torch, build, runs), res["sent_in_front"])
    bc = rtcp.count("build", bcnt)
    assert bc["built"] == N and bc["with_sr"] == N, bc
    res["a_build_trailer_0"]["bytes_per_packet"] = bc["bytes"] / N
    plain_d, plain_w = rd.clone(), rw.clone()                              # (c) parses these
    rtcp.set_trailer(solo_amd.SRTCP_TRAILER_BYTES)
    res["a_build_trailer_14"] = minus(timed(torch, build, runs), res["sent_in_front"])
    bc = rtcp.count("build", bcnt)
    assert bc["built"] == N, bc
    res["a_build_trailer_14"]["bytes_per_packet"] = bc["bytes"] / N
    # (b) build + protect
    both = minus(timed(torch, build_protect, runs), res["sent_in_front"])
    pc = theirs.srtcp_count(scnt)
    assert pc["ok"] == N, pc
    res["b_build_and_protect"] = both
    res["b_protect"] = minus(both, res["a_build_trailer_14"])
    res["b_protect"]["bytes_per_packet"] = float(rd[:, 1].sum().item()) / N
    # (c) parse alone, in the clear
    fb, qcnt, ucnt = z((N, 8), torch.int32), z((16,), torch.int32), z((8,), torch.int32)
    res["c_parse"] = timed(torch, lambda: L.solo_rtcp_parse(peer.h, theirs.h, ours.h, plain_d.data_ptr(), N, plain_w.data_ptr(), CAP, now + (1 << 32), None,
                                                            fb.data_ptr(), qcnt.data_ptr(), st), runs)
    q = peer.count("parse", qcnt)
    assert q["accepted"] == N and q["sr"] == N and q["blocks"] == N, q
    # (d) unprotect + parse: BATCHES protected batches with rising indices; a call works on a copy (unprotect decrypts in place), the copy is
    # timed alone and taken off; the receive records are set back between the windows, which is where a window's first batch is new again
    batches = []
    theirs.set_rtcp_keys(range(N), tx=master, tx_index=0)
    for _ in range(BATCHES):
        assert build_protect() == 0
        batches.append((rd.clone(), rw.clone()))
    work, out = z((CAP,), torch.uint8), z((N, 2), torch.int32)
    at = [0]

    def step():
        at[0] = (at[0] + 1) % BATCHES
        return batches[at[0]]

    def copy_only():
        work.copy_(step()[1])
        return 0

    def unprotect_parse():
        d, w = step()
        work.copy_(w)
        r = L.solo_srtcp_unprotect(theirs.h, d.data_ptr(), N, work.data_ptr(), CAP, out.data_ptr(), ucnt.data_ptr(), st)
        return r or L.solo_rtcp_parse(peer.h, theirs.h, ours.h, out.data_ptr(), N, work.data_ptr(), CAP, now + (1 << 32), None, fb.data_ptr(), qcnt.data_ptr(), st)
    res["d_copy"] = timed(torch, copy_only, runs)
    theirs.set_rtcp_keys(range(N), rx=master, rx_index=-1)
    at[0] = -1
    assert unprotect_parse() == 0
    u = theirs.srtcp_count(ucnt)
    assert u["ok"] == N and peer.count("parse", qcnt)["accepted"] == N, u
    accepted = []
    torch.cuda.synchronize()
    for _ in range(runs):                                                  # windows of exactly BATCHES calls, every datagram accepted
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        theirs.set_rtcp_keys(range(N), rx=master, rx_index=-1)
        at[0] = -1
        e0.record()
        for _ in range(BATCHES):
            unprotect_parse()
        e1.record()
        torch.cuda.synchronize()
        accepted.append(e0.elapsed_time(e1) / BATCHES)
        u = theirs.srtcp_count(ucnt)
        assert u["ok"] == N, u
    accepted.sort()
    both = {"ms": round(accepted[len(accepted) // 2], 5), "min_ms": round(accepted[0], 5), "max_ms": round(accepted[-1], 5), "iters": BATCHES}
    res["d_copy_unprotect_parse_accepted"] = both
    res["d_unprotect_accepted"] = minus(minus(both, res["d_copy"]), res["c_parse"])
    res["d_unprotect_accepted"]["bytes_per_packet"] = float(batches[0][0][:, 1].sum().item()) / N
    res["d_copy_unprotect_parse_replayed"] = timed(torch, unprotect_parse, runs)       # the records stand at the last batch: everything is old
    u = theirs.srtcp_count(ucnt)
    assert u["replayed"] + u["ok"] == N, u
    res["ratios"] = {"protect_over_build": round(res["b_protect"]["ms"] / res["a_build_trailer_14"]["ms"], 3),
                     "unprotect_over_parse": round(res["d_unprotect_accepted"]["ms"] / res["c_parse"]["ms"], 3),
                     "build_trailer_14_over_0": round(res["a_build_trailer_14"]["ms"] / res["a_build_trailer_0"]["ms"], 3)}
    for o in (rtcp, peer, ours, theirs):
        o.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--out")
    ap.add_argument("--rtcp-before")
    ap.add_argument("--rtcp-after")
    a = ap.parse_args()
    import torch
    res = {"runs": a.runs, "kernel_source_hash": solo_amd.kernel_source_hash(), "shader_clock_mhz_before": solo_amd.shader_clock_mhz()}
    res.update(run(torch, a.streams, a.runs))
    res["shader_clock_mhz_after"] = solo_amd.shader_clock_mhz()
    if a.rtcp_before and a.rtcp_after:
        pick = lambda path: [dict(packets=s["packets"], **{k: s["c_build"][k] for k in ("ms", "min_ms", "max_ms")}) for s in json.load(open(path))["shapes"]]
        res["rtcp_bench_c_build_trailer_0"] = {"parent": pick(a.rtcp_before), "this": pick(a.rtcp_after)}
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()

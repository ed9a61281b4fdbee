#!/usr/bin/env python3
"""Cost of the read side of the receiver ring (solo_recv_report, solo_recv_track) at 4096 streams, 13.6 kbps, ring depth 8 and 64,
HIP-event medians of 7 after a warm-up:

  (a) one solo_recv_report of all streams: reports + play-out list + count
  (b) a plain device copy of max(N x depth x 4 bytes read, N x 64 + N x 8 bytes written): the floor of (a)
  (c) the one-packet receive tick -- solo_recv_insert of 2N arrivals + solo_recv_decode -- with tracking off
  (d) the same tick with tracking on
  (e) (c) measured on the PARENT commit, twice: the baseline and its run-to-run spread.  This script cannot check out another commit;
      run it with --tick-only --package-root <a built checkout of the parent> --out <file> twice and hand the files to --parent.

  python tools/recv_report_bench.py [--streams 4096] [--depths 8 64] [--runs 7] [--parent e1.json e2.json] [--out profiles/recv_report.json]
"""
import argparse
import json
import os
import sys

import numpy as np


def timed(torch, fn, runs):
    """fn(r) for r = 0 .. runs; run 0 is the warm-up"""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for r in range(runs + 1):
        torch.cuda.synchronize()
        ev[0].record()
        fn(r)
        ev[1].record()
        torch.cuda.synchronize()
        if r:
            ms.append(ev[0].elapsed_time(ev[1]))
    return {"ms": float(np.median(ms)), "runs_ms": [round(x, 4) for x in ms]}


def pool(torch, solo_amd, n_src, P):
    """n_src x P packets encoded on the device -> (payload pool, offsets / lengths [n_src, P, 2])"""
    from solo_amd.synth import synth_stream
    pcm = torch.from_numpy(np.stack([synth_stream(i, P) for i in range(n_src)]).reshape(n_src, P, 640)).cuda()
    e = solo_amd.SoloBatch(n_src, rate=13600, encoder=True, decoder=False, slot_bytes=512)
    bits, nb, _ = e.encode(pcm)
    torch.cuda.synchronize()
    hb, hn = bits.cpu().numpy(), nb.cpu().numpy()
    e.close()
    off, ln, blobs, o = np.zeros((n_src, P, 2), np.int64), np.zeros((n_src, P, 2), np.int64), [], 0
    for i in range(n_src):
        for p in range(P):
            n0, n1 = int(hn[i, p, 0]), int(hn[i, p, 1])
            for d, part in enumerate((hb[i, p, :n0 - n1], hb[i, p, n0 - n1:n0])):
                off[i, p, d], ln[i, p, d] = o, part.size
                blobs.append(part)
                o += part.size
    return torch.from_numpy(np.concatenate(blobs)).cuda(), off, ln


def tick_arrivals(torch, N, n_src, P, off, ln):
    """per tick t < P: both descriptions of packet t of every stream (stream s carries source s mod n_src)"""
    out = []
    s = np.arange(N)
    for t in range(P):
        a = np.zeros((N, 2, 5), np.int32)
        for d in (0, 1):
            a[:, d, 0], a[:, d, 1], a[:, d, 2] = s, t, d
            a[:, d, 3], a[:, d, 4] = off[s % n_src, t, d], ln[s % n_src, t, d]
        out.append(torch.from_numpy(a.reshape(2 * N, 5)).cuda())
    return out


def tick(torch, solo_amd, N, depth, runs, payload, arrivals, track):
    b = solo_amd.SoloBatch(N, rate=13600, encoder=False, decoder=True, slot_bytes=512)
    b.recv_create(depth, 256, 0)
    if track:
        b.recv_track(True)
    pcm = torch.zeros((N, 1, 640), dtype=torch.int16, device="cuda")
    st = torch.zeros((N,), dtype=torch.int32, device="cuda")

    def fn(r):
        b.recv_insert(arrivals[r], payload)
        b.recv_decode(1, pcm=pcm, status=st)
    res = timed(torch, fn, runs)
    assert int(st.abs().max()) == 0 and b.recv_stats()["inserted"] == 2 * N * (runs + 1)
    b.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--depths", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--tick-only", action="store_true", help="measure (c) alone, with the calls every earlier version of the package has")
    ap.add_argument("--package-root", help="import solo_amd from this checkout instead of the one this script lies in")
    ap.add_argument("--parent", nargs="*", default=[], help="--tick-only results of the parent commit: become (e)")
    ap.add_argument("--out")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root) if a.package_root else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import solo_amd
    N, n_src, P = a.streams, 64, a.runs + 1
    res = {"runs": a.runs, "streams": N, "kernel_source_hash": solo_amd.kernel_source_hash(), "shader_clock_mhz_before": solo_amd.shader_clock_mhz(),
           "depths": []}
    payload, off, ln = pool(torch, solo_amd, n_src, P)
    arrivals = tick_arrivals(torch, N, n_src, P, off, ln)
    for depth in a.depths:
        r = {"depth": depth, "c_tick_track_off": tick(torch, solo_amd, N, depth, a.runs, payload, arrivals, False)}
        if not a.tick_only:
            r["d_tick_track_on"] = tick(torch, solo_amd, N, depth, a.runs, payload, arrivals, True)
            b = solo_amd.SoloBatch(N, rate=13600, encoder=False, decoder=True, slot_bytes=512)
            b.recv_create(depth, 256, 0)
            b.recv_track(True)
            for t in range(min(P, depth) - 1, -1, -1):        # a queue that is filled from the back: every report walks the whole depth
                b.recv_insert(arrivals[t][::2 if t % 2 else 1].contiguous(), payload)
            rep, lst, rows, cnt = b.recv_report(min_ready=2)
            r["selected"] = b.recv_report_count(cnt)["selected"]
            r["a_recv_report"] = timed(torch, lambda _: b.recv_report(min_ready=2, reports=rep, play_list=lst, play_rows=rows), a.runs)
            nbytes = max(N * depth * 4, N * 64 + N * 8)
            src, dst = torch.zeros(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            r["b_d2d_copy"] = timed(torch, lambda _: dst.copy_(src), a.runs)
            r["b_d2d_copy"]["bytes"] = nbytes
            b.close()
            r["a_over_b"] = round(r["a_recv_report"]["ms"] / r["b_d2d_copy"]["ms"], 3)
            r["d_minus_c_ms"] = round(r["d_tick_track_on"]["ms"] - r["c_tick_track_off"]["ms"], 5)
            r["a_over_c"] = round(r["a_recv_report"]["ms"] / r["c_tick_track_off"]["ms"], 4)
        res["depths"].append(r)
    res["shader_clock_mhz_after"] = solo_amd.shader_clock_mhz()
    if a.parent:
        res["e_parent_tick"] = [json.load(open(p)) for p in a.parent]
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()

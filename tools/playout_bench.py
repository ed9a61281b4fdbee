#!/usr/bin/env python3
"""Cost of the play-out delay control (solo_playout_tick) at 4096 streams, 13.6 kbps, ring depth 8, one packet per tick, through the
binding, HIP-event medians of 7 after a warm-up.  Four packets per stream are queued ahead; one more per stream is filed ahead of
every tick, outside the timed region.

  (a) solo_playout_tick with every row NORMAL (lo = 0, hi = 64)
  (b) the tick by hand, with calls every earlier version of the package has: recv_report with a list, the 8-byte count read,
      recv_decode(1, streams=...)
  (c) (a) with 5 % of the rows stretching and 5 % accelerating in every tick (their records are set ahead of the tick, outside the timed
      region; another twentieth each tick, and a row that has moved cools down for the rest of the run)
  (d) plan and render alone (every row NORMAL)
  (e) (b) measured on the PARENT commit, twice: the baseline and its run-to-run spread.  This script cannot check out another commit; run it
      with --by-hand-only --package-root <a built checkout of the parent> --out <file> twice and hand the files to --parent.

What to expect: (a) - (b) is the launches of plan and render plus one pass over N x L x 2 bytes.

  python tools/playout_bench.py [--streams 4096] [--runs 7] [--parent e1.json e2.json] [--out profiles/playout.json]
"""
import argparse
import json
import os
import sys

import numpy as np

DEPTH, AHEAD, L = 8, 4, 640


def timed(torch, fn, runs, prep=None):
    """prep(r) untimed, then fn(r) timed, for r = 0 .. runs; run 0 is the warm-up"""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for r in range(runs + 1):
        if prep:
            prep(r)
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
    pcm = torch.from_numpy(np.stack([synth_stream(i, P) for i in range(n_src)]).reshape(n_src, P, L)).cuda()
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


def packet_arrivals(torch, N, n_src, P, off, ln):
    """per packet t < P: both descriptions of packet t of every stream (stream s carries source s mod n_src)"""
    out = []
    s = np.arange(N)
    for t in range(P):
        a = np.zeros((N, 2, 5), np.int32)
        for d in (0, 1):
            a[:, d, 0], a[:, d, 1], a[:, d, 2] = s, t, d
            a[:, d, 3], a[:, d, 4] = off[s % n_src, t, d], ln[s % n_src, t, d]
        out.append(torch.from_numpy(a.reshape(2 * N, 5)).cuda())
    return out


def handle(torch, solo_amd, N, payload, arrivals):
    b = solo_amd.SoloBatch(N, rate=13600, encoder=False, decoder=True, slot_bytes=512)
    b.recv_create(DEPTH, 256, 0)
    b.recv_track(True)
    for t in range(AHEAD):
        b.recv_insert(arrivals[t], payload)
    return b


def by_hand(torch, solo_amd, N, runs, payload, arrivals):
    b = handle(torch, solo_amd, N, payload, arrivals)
    streams = torch.arange(N, dtype=torch.int32, device="cuda")
    rep, lst, rows = (torch.zeros(s, dtype=torch.int32, device="cuda") for s in ((N, 16), (N,), (N,)))
    pcm, st = torch.zeros((N, 1, L), dtype=torch.int16, device="cuda"), torch.zeros((N,), dtype=torch.int32, device="cuda")

    def fn(r):
        _, _, _, cnt = b.recv_report(streams=streams, min_ready=1, clear_margin=True, reports=rep, play_list=lst, play_rows=rows)
        k = b.recv_report_count(cnt)["selected"]
        assert k == N
        b.recv_decode(1, pcm=pcm, status=st, streams=lst[:k])
    res = timed(torch, fn, runs, lambda r: b.recv_insert(arrivals[AHEAD + r], payload))
    assert int(st.abs().max()) == 0
    b.close()
    return res


def crafted(N, r, value):
    """state records [k][128 + 2 L] of running rows whose ring holds `value` everywhere, for the rows r mod 20 of every 20"""
    rows = np.arange(r % 20, N, 20, dtype=np.int32)
    rec = np.zeros((len(rows), 32 + L // 2), np.int32)
    rec[:, 0], rec[:, 4] = 1, 8                                 # run, age = the window
    rec[:, 8:24] = np.array([value, value], np.int16).view(np.int32)[0]
    return rows, rec.view(np.uint8).reshape(len(rows), -1)


def ticks(torch, solo_amd, N, runs, payload, arrivals, moving):
    b = handle(torch, solo_amd, N, payload, arrivals)
    po = solo_amd.Playout(N, L)
    prm = dict(start_ready=1, max_span=0, window=8, tolerate=1, lo=1, hi=16, cooldown=1000, cost_gate=0) if moving else \
        dict(start_ready=1, max_span=0, window=8, tolerate=1, lo=0, hi=64, cooldown=0, cost_gate=0)
    po.tick(b, **prm)                                           # every row starts
    b.recv_insert(arrivals[AHEAD], payload)
    counts = []

    def prep(r):
        b.recv_insert(arrivals[AHEAD + 1 + r], payload)
        if moving:
            for shift, value in ((0, -5), (10, 100)):           # a ring of -5: too short, stretch; of 100: too long, accelerate
                rows, rec = crafted(N, r + shift, value)
                po.set_state(torch.from_numpy(rec).cuda(), rows=torch.from_numpy(rows).cuda())

    def fn(r):
        counts.append(po.tick(b, **prm)[3])
    res = timed(torch, fn, runs, prep)
    res["outcomes"] = [po.count(c)["render"] for c in counts][-1]
    want = N // 20 if moving else 0
    assert all(abs(po.count(c)["render"][k] - want) <= 1 for c in counts[1:] for k in ("stretch", "accel")), res["outcomes"]
    b.close()
    return res


def stages(torch, solo_amd, N, runs, payload, arrivals):
    b = handle(torch, solo_amd, N, payload, arrivals)
    po = solo_amd.Playout(N, L)
    prm = dict(start_ready=1, max_span=0, window=8, tolerate=1, lo=0, hi=64, cooldown=0, cost_gate=0)
    rep = b.recv_report(clear_margin=True)[0]
    pl = po.plan(rep, DEPTH, **prm)
    assert po.count(pl["count"])["n_one"] == N
    pcm, st = b.recv_decode(1, streams=pl["one"])
    one = pcm[:, 0].contiguous()
    return {"plan": timed(torch, lambda r: po.plan(rep, DEPTH, **prm), runs),
            "render": timed(torch, lambda r: po.render(pl["action"], 80, pcm_one=one, status_one=st, **prm), runs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--by-hand-only", action="store_true", help="measure (b) alone, with the calls every earlier version of the package has")
    ap.add_argument("--package-root", help="import solo_amd from this checkout instead of the one this script lies in")
    ap.add_argument("--parent", nargs="*", default=[], help="--by-hand-only results of the parent commit: become (e)")
    ap.add_argument("--out")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root) if a.package_root else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import solo_amd
    N, n_src, P = a.streams, 64, a.runs + 2 + AHEAD
    res = {"runs": a.runs, "streams": N, "depth": DEPTH, "kernel_source_hash": solo_amd.kernel_source_hash(),
           "shader_clock_mhz_before": solo_amd.shader_clock_mhz()}
    payload, off, ln = pool(torch, solo_amd, n_src, P)
    arrivals = packet_arrivals(torch, N, n_src, P, off, ln)
    res["b_by_hand"] = by_hand(torch, solo_amd, N, a.runs, payload, arrivals)
    if not a.by_hand_only:
        res["a_tick_all_normal"] = ticks(torch, solo_amd, N, a.runs, payload, arrivals, False)
        res["c_tick_5pct_stretch_5pct_accel"] = ticks(torch, solo_amd, N, a.runs, payload, arrivals, True)
        res["d_stages"] = stages(torch, solo_amd, N, a.runs, payload, arrivals)
        res["a_minus_b_ms"] = round(res["a_tick_all_normal"]["ms"] - res["b_by_hand"]["ms"], 5)
        res["c_minus_a_ms"] = round(res["c_tick_5pct_stretch_5pct_accel"]["ms"] - res["a_tick_all_normal"]["ms"], 5)
    res["shader_clock_mhz_after"] = solo_amd.shader_clock_mhz()
    if a.parent:
        res["e_parent_by_hand"] = [json.load(open(p)) for p in a.parent]
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()

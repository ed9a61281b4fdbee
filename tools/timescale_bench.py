#!/usr/bin/env python3
"""Cost of play-out time scaling (solo_timescale) at 4096 rows, 16 kHz and 32 kHz (40 ms packets), ratios 2 -> 1, 3 -> 2 and 1 -> 2,
HIP-event medians after a warm-up, next to, in the same run:

  (a) one solo_timescale of PCM the receiver played out
  (b) a plain device copy with the same traffic: a tensor of (in + out) / 2 packets per row, read once and written once
  (c) the one-packet solo_recv_decode of the same rows that the call follows (encoded packets out of the ring)

  python tools/timescale_bench.py [--rows 4096] [--runs 7] [--out profiles/timescale.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import solo_amd                       # noqa: E402
from solo_amd.synth import synth_stream  # noqa: E402

RATIOS = ((2, 1), (3, 2), (1, 2))


def timed(torch, fn, runs):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for r in range(runs + 1):                       # (the first run is a warm-up)
        torch.cuda.synchronize()
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        if r:
            ms.append(ev[0].elapsed_time(ev[1]))
    return {"ms": float(np.median(ms)), "runs_ms": [round(x, 4) for x in ms]}


def rate(torch, N, fs, runs):
    P = runs + 1                                    # one packet per timed play-out
    x = np.stack([synth_stream(i % 64, P) for i in range(N)]).reshape(N, P, 640)
    if fs == 32000:
        x = np.repeat(x, 2, axis=2)                 # (the 16 kHz signal an octave down: the cost of a play-out hardly depends on it)
    tx = solo_amd.SoloBatch(N, rate=13600 if fs == 16000 else 24000, encoder=True, decoder=False, slot_bytes=512, samplerate=fs)
    bits, nb, st = tx.encode(torch.from_numpy(x).cuda())
    rec, pay, cnt = tx.send_pack(bits, nb)
    c = tx.send_count(cnt)
    assert int(st.abs().max()) == 0 and c["refused"] == 0 and c["records"] == c["records_needed"] > 0, c
    tx.close()
    rx = solo_amd.SoloBatch(N, encoder=False, decoder=True, samplerate=fs)
    L = rx.packet_samples
    rx.recv_create(P, 256, 0)
    rx.recv_insert(rec[:c["records"]].contiguous(), pay)
    played = []

    def play():
        played.append(rx.recv_decode(1)[0])
    res = {"samplerate": fs, "rows": N, "packet_samples": L, "c_recv_decode": timed(torch, play, runs), "ratios": []}
    heard = torch.cat(played[-3:], dim=1).contiguous()          # [N, 3, L]: what the receiver played last
    for a, b in RATIOS:
        pcm = heard[:, :a].contiguous()
        out = torch.empty((N, b, L), dtype=torch.int16, device="cuda")
        _, count = rx.timescale(pcm, b, out=out)
        cc = rx.timescale_count(count)
        assert cc["rows"] == N, cc
        t = timed(torch, lambda: rx.timescale(pcm, b, out=out), runs)
        src = torch.zeros((N * (a + b) * L // 2,), dtype=torch.int16, device="cuda")
        dst = torch.empty_like(src)
        cp = timed(torch, lambda: dst.copy_(src), runs)
        res["ratios"].append({"in_packets": a, "out_packets": b, "count": cc, "bytes_read_and_written": int(N * (a + b) * L * 2),
                              "mean_cost_per_searched_block": round(cc["cost"] / max(cc["blocks"], 1), 1), "a_timescale": t, "b_copy": cp,
                              "a_over_b": round(t["ms"] / cp["ms"], 3), "a_over_c": round(t["ms"] / res["c_recv_decode"]["ms"], 5)})
    rx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    res = {"runs": a.runs, "kernel_source_hash": solo_amd.kernel_source_hash(), "shader_clock_mhz_before": solo_amd.shader_clock_mhz(), "rates": []}
    for fs in (16000, 32000):
        res["rates"].append(rate(torch, a.rows, fs, a.runs))
    res["shader_clock_mhz_after"] = solo_amd.shader_clock_mhz()
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()

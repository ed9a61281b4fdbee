#!/usr/bin/env python3
"""Cost of the mixing bridge (solo_mix) at 4096 rows x 1 and x 50 packets, 16 kHz, HIP-event medians after a warm-up, for three floors:
rooms of 2, rooms of 8, and one room of 4096 -- each with max_speakers 3:

  (a) one solo_mix
  (b) a plain device copy of the same PCM (out.copy_(pcm)): two row-sizes of traffic where the mix moves at most three
  (c) the encode call the mix feeds, for scale

  python tools/mix_bench.py [--rows 4096] [--packets 1 50] [--runs 7] [--out profiles/mix.json]
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


def shape(torch, N, P, runs, max_speakers):
    pcm = torch.from_numpy(np.stack([synth_stream(i % 64, P) for i in range(N)]).reshape(N, P, 640)).cuda()
    b = solo_amd.SoloBatch(N, rate=13600, encoder=True, decoder=False, slot_bytes=512)
    out = torch.zeros_like(pcm)
    res = {"rows": N, "packets": P, "max_speakers": max_speakers, "pcm_bytes": int(pcm.numel() * 2)}
    res["b_copy"] = timed(torch, lambda: out.copy_(pcm), runs)
    bits, nb, _ = b.encode(pcm)

    def enc():
        b.reset()
        b.encode(pcm, bits=bits, nbytes=nb)
    rst = timed(torch, b.reset, runs)
    res["c_encode"] = timed(torch, enc, runs)
    res["c_encode"]["ms"] = res["c_encode"]["ms"] - rst["ms"]
    res["c_encode"]["reset_ms"] = rst["ms"]
    res["floors"] = []
    perm = np.random.default_rng(1).permutation(N)
    for name, size in (("rooms_of_2", 2), ("rooms_of_8", 8), ("one_room", N)):
        room = torch.from_numpy((perm // size).astype(np.int32)).cuda()
        _, count = b.mix(pcm, room, max_speakers=max_speakers, out=out)
        c = b.mix_count(count)
        assert c["rows"] == N and c["rooms"] == N // size, c
        a = timed(torch, lambda: b.mix(pcm, room, max_speakers=max_speakers, out=out), runs)
        res["floors"].append({"floor": name, "count": c, "a_mix": a, "a_over_b": round(a["ms"] / res["b_copy"]["ms"], 3),
                              "a_over_c": round(a["ms"] / res["c_encode"]["ms"], 5)})
    b.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--packets", type=int, nargs="+", default=[1, 50])
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--max-speakers", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    res = {"runs": a.runs, "kernel_source_hash": solo_amd.kernel_source_hash(), "shader_clock_mhz_before": solo_amd.shader_clock_mhz(), "shapes": []}
    for P in a.packets:
        res["shapes"].append(shape(torch, a.rows, P, a.runs, a.max_speakers))
    res["shader_clock_mhz_after"] = solo_amd.shader_clock_mhz()
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()

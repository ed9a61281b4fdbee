#!/usr/bin/env python3
"""Cost of the PCM resampler (solo_resample) at 4096 rows x 1 and x 50 packets of 40 ms, every pair, HIP-event medians after a
warm-up, next to the stage that stands beside it in the bridge tick: one solo_mix of the same rows and packets with every member
mixed (rooms of 8, max_speakers 0), on a 16 kHz and on a 32 kHz handle.  solo_mix is measured in the same process, so both numbers
come from the same GPU and session.

  python tools/resample_bench.py [--rows 4096] [--packets 1 50] [--runs 7] [--out profiles/resample.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import solo_amd                       # noqa: E402


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


def speechlike(torch, shape, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randint(-3000, 3001, shape, generator=g, device="cuda", dtype=torch.int32).to(torch.int16)


def mix_ms(torch, N, P, samplerate, runs):
    L = 640 * samplerate // 16000
    b = solo_amd.SoloBatch(N, rate=15600, encoder=False, decoder=True, samplerate=samplerate)
    pcm = speechlike(torch, (N, P, L), 7)
    out = torch.zeros_like(pcm)
    room = torch.from_numpy((np.random.default_rng(1).permutation(N) // 8).astype(np.int32)).cuda()
    _, count = b.mix(pcm, room, max_speakers=0, out=out)
    c = b.mix_count(count)
    assert c["rows"] == N, c
    res = timed(torch, lambda: b.mix(pcm, room, max_speakers=0, out=out), runs)
    res["per_row_packet_us"] = res["ms"] * 1e3 / (N * P)
    b.close()
    return res


def pair_ms(torch, N, P, fs_in, fs_out, runs):
    rs = solo_amd.Resampler(N, fs_in, fs_out)
    L = fs_in // 1000 * 40
    pcm = speechlike(torch, (N, P, L), 11)
    out = torch.zeros((N, P, rs.out_samples(L)), dtype=torch.int16, device="cuda")
    res = timed(torch, lambda: rs.run(pcm, out=out), runs)
    res["per_row_packet_us"] = res["ms"] * 1e3 / (N * P)
    res["bytes"] = int(pcm.numel() * 2 + out.numel() * 2)
    res["gbytes_per_s"] = res["bytes"] / (res["ms"] * 1e-3) / 1e9
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--packets", type=int, nargs="+", default=[1, 50])
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    res = {"runs": a.runs, "kernel_source_hash": solo_amd.kernel_source_hash(), "shader_clock_mhz_before": solo_amd.shader_clock_mhz(),
           "rows_per_workgroup": 16, "shapes": []}
    for P in a.packets:
        sh = {"rows": a.rows, "packets": P, "packet_ms": 40,
              "mix_16k": mix_ms(torch, a.rows, P, 16000, a.runs), "mix_32k": mix_ms(torch, a.rows, P, 32000, a.runs), "pairs": []}
        for fs_in, fs_out in solo_amd.RESAMPLE_PAIRS:
            r = pair_ms(torch, a.rows, P, fs_in, fs_out, a.runs)
            r["pair"] = "%d->%d" % (fs_in, fs_out)
            r["over_mix_16k"] = round(r["ms"] / sh["mix_16k"]["ms"], 3)
            r["over_mix_32k"] = round(r["ms"] / sh["mix_32k"]["ms"], 3)
            sh["pairs"].append(r)
        res["shapes"].append(sh)
    res["shader_clock_mhz_after"] = solo_amd.shader_clock_mhz()
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()

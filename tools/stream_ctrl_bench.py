#!/usr/bin/env python3
"""Cost of per-stream controls: 4096 streams x 50 packets encoded and decoded twice on the same PCM, once with one uniform control
(13600 bps, no DTX, useMDIndex 0: the benchmark's) and once with mixed controls given per stream through solo_batch_reset_streams
(cycling {13600, 15600, 24000} bps x DTX off / on x useMDIndex 0 / 1).  Encode-only and decode-only times are HIP-event medians of
several runs; every run starts from freshly reset streams.

  python tools/stream_ctrl_bench.py [--streams 4096] [--packets 50] [--runs 7] [--out FILE]
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

COMBOS = [(r, d, m) for r in (13600, 15600, 24000) for d in (0, 1) for m in (0, 1)]


def run(torch, pcm, mixed, runs, combos=COMBOS):
    """mixed = False: the handle's own control (solo_batch_reset); True: per-stream controls cycling over `combos`"""
    N, P, _ = pcm.shape
    b = solo_amd.SoloBatch(N, rate=13600, encoder=True, decoder=True, slot_bytes=512)
    ctl = [combos[i % len(combos)] for i in range(N)]

    def reset():
        if mixed:
            b.reset_streams(range(N), rate=[c[0] for c in ctl], dtx=[c[1] for c in ctl], use_md_index=[c[2] for c in ctl])
        else:
            b.reset()

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    enc_ms, dec_ms, empty = [], [], 0
    for r in range(runs + 1):                       # (the first run is a warm-up)
        reset()
        torch.cuda.synchronize()
        ev[0].record()
        bits, nb, _ = b.encode(pcm)
        ev[1].record()
        b.decode(bits, nb, None)
        ev[2].record()
        torch.cuda.synchronize()
        if r:
            enc_ms.append(ev[0].elapsed_time(ev[1]))
            dec_ms.append(ev[1].elapsed_time(ev[2]))
        empty = int((nb[:, :, 0] == 0).sum())
    b.close()
    return {"encode_ms": float(np.median(enc_ms)), "decode_ms": float(np.median(dec_ms)), "encode_runs_ms": [round(x, 3) for x in enc_ms],
            "decode_runs_ms": [round(x, 3) for x in dec_ms], "empty_dtx_packets": empty}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--packets", type=int, default=50)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    pcm = torch.from_numpy(np.stack([synth_stream(i, a.packets) for i in range(a.streams)]).reshape(a.streams, a.packets, 640)).cuda()
    res = {"streams": a.streams, "packets": a.packets, "runs": a.runs, "kernel_source_hash": solo_amd.kernel_source_hash(),
           "shader_clock_mhz_before": solo_amd.shader_clock_mhz()}
    # alternate the order so that a drifting clock does not favour one side
    res["uniform"] = run(torch, pcm, False, a.runs)
    res["mixed"] = run(torch, pcm, True, a.runs)
    res["uniform_again"] = run(torch, pcm, False, a.runs)
    # what the mixed figures are made of: the uniform control given to every stream through the per-stream path (the mechanism alone),
    # then one factor of the mix at a time (the work each configuration asks for)
    res["uniform_given_per_stream"] = run(torch, pcm, True, a.runs, [(13600, 0, 0)])
    res["rates_only"] = run(torch, pcm, True, a.runs, [(13600, 0, 0), (15600, 0, 0), (24000, 0, 0)])
    res["dtx_only"] = run(torch, pcm, True, a.runs, [(13600, 0, 0), (13600, 1, 0)])
    res["md_index_only"] = run(torch, pcm, True, a.runs, [(13600, 0, 0), (13600, 0, 1)])
    res["shader_clock_mhz_after"] = solo_amd.shader_clock_mhz()
    u_enc = min(res["uniform"]["encode_ms"], res["uniform_again"]["encode_ms"])
    u_dec = min(res["uniform"]["decode_ms"], res["uniform_again"]["decode_ms"])
    for k in ("mixed", "uniform_given_per_stream", "rates_only", "dtx_only", "md_index_only"):
        res[k + "_vs_uniform"] = {"encode": round(res[k]["encode_ms"] / u_enc - 1.0, 4), "decode": round(res[k]["decode_ms"] / u_dec - 1.0, 4)}
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()

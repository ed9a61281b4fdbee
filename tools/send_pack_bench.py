#!/usr/bin/env python3
"""Cost of the sender back end (solo_send_pack) at 4096 streams x 1 and x 50 packets, 13.6 kbps, HIP-event medians after a warm-up:

  (a) one solo_send_pack (every description of every packet sent)
  (b) a device-to-device copy of the `bytes` it wrote: the bandwidth floor of the copy
  (c) a device-to-host copy of the whole slot array plus the length records into pinned memory: what a caller had to do before
  (d) a device-to-host copy of the records, the `bytes` of payload and the count: what it has to do now
  (e) the encode call of the same shape, for scale

  python tools/send_pack_bench.py [--streams 4096] [--packets 1 50] [--runs 7] [--out profiles/send_pack.json]
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


def shape(torch, N, P, runs):
    pcm = torch.from_numpy(np.stack([synth_stream(i % 64, P) for i in range(N)]).reshape(N, P, 640)).cuda()
    b = solo_amd.SoloBatch(N, rate=13600, encoder=True, decoder=False, slot_bytes=512)
    bits, nb, _ = b.encode(pcm)
    records, payload, count = b.send_pack(bits, nb)
    c = b.send_count(count)
    assert c["records"] == c["records_needed"] and c["bytes"] == c["bytes_needed"] and c["refused"] == 0
    nrec, nbytes = c["records"], c["bytes"]
    res = {"streams": N, "packets": P, "count": c, "mean_packet_bytes": round(nbytes / max(1, N * P - c["empty"]), 2)}
    res["a_send_pack"] = timed(torch, lambda: b.send_pack(bits, nb, records=records, payload=payload), runs)
    dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    res["b_d2d_bytes"] = timed(torch, lambda: dst.copy_(payload[:nbytes]), runs)
    h_bits = torch.empty(bits.shape, dtype=torch.uint8).pin_memory()
    h_nb = torch.empty(nb.shape, dtype=torch.int16).pin_memory()
    res["c_d2h_slots"] = timed(torch, lambda: (h_bits.copy_(bits, non_blocking=True), h_nb.copy_(nb, non_blocking=True)), runs)
    res["c_d2h_slots"]["bytes"] = int(bits.numel() + 2 * nb.numel())
    h_rec = torch.empty((nrec, 5), dtype=torch.int32).pin_memory()
    h_pay = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
    h_cnt = torch.empty(8, dtype=torch.int32).pin_memory()
    res["d_d2h_packed"] = timed(torch, lambda: (h_rec.copy_(records[:nrec], non_blocking=True), h_pay.copy_(payload[:nbytes], non_blocking=True),
                                                h_cnt.copy_(count, non_blocking=True)), runs)
    res["d_d2h_packed"]["bytes"] = int(20 * nrec + nbytes + 32)

    def enc():
        b.reset()
        b.encode(pcm, bits=bits, nbytes=nb)
    rst = timed(torch, b.reset, runs)
    res["e_encode"] = timed(torch, enc, runs)
    res["e_encode"]["ms"] = res["e_encode"]["ms"] - rst["ms"]
    res["e_encode"]["reset_ms"] = rst["ms"]
    a = res["a_send_pack"]["ms"]
    res["ratios"] = {"a_over_b": round(a / res["b_d2d_bytes"]["ms"], 3), "a_over_e": round(a / res["e_encode"]["ms"], 5),
                     "c_over_d": round(res["c_d2h_slots"]["ms"] / res["d_d2h_packed"]["ms"], 3)}
    b.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--packets", type=int, nargs="+", default=[1, 50])
    ap.add_argument("--runs", type=int, default=7)
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

#!/usr/bin/env python3
"""Cost of the VAD stage (solo_vad, solo_vad_select) at 4096 rows x 1 and x 50 packets of 40 ms at 16 kHz (frames of 320 samples),
HIP-event medians after a warm-up, next to what stands beside it in the bridge tick, measured in the same process:

  a  solo_vad                       activities + levels of the rows (with P packets: P packets per row in one call)
  b  solo_vad_select                rooms of 8, and one room of all rows
  c  a device copy of the same PCM  the floor of anything that reads the rows once
  d  solo_recv_decode               the one-packet play-out of the same rows
  e  solo_mix                       one mix of them (rooms of 8, every member mixed)

  python tools/vad_bench.py [--rows 4096] [--packets 1 50] [--runs 7] [--out profiles/vad.json]
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


def played_rows(torch, N, runs):
    """(d): N streams encoded, queued and played one packet per timed call -> (timing, the last packet played int16 [N, 1, 640])"""
    P = runs + 1
    base = [synth_stream(i, P) for i in range(64)]
    x = np.stack([base[i % 64] for i in range(N)]).reshape(N, P, 640)
    tx = solo_amd.SoloBatch(N, rate=13600, encoder=True, decoder=False, slot_bytes=512)
    bits, nb, st = tx.encode(torch.from_numpy(x).cuda())
    rec, pay, cnt = tx.send_pack(bits, nb)
    c = tx.send_count(cnt)
    assert int(st.abs().max()) == 0 and c["refused"] == 0 and c["records"] == c["records_needed"] > 0, c
    tx.close()
    rx = solo_amd.SoloBatch(N, encoder=False, decoder=True)
    rx.recv_create(P, 256, 0)
    rx.recv_insert(rec[:c["records"]].contiguous(), pay)
    played = []
    t = timed(torch, lambda: played.append(rx.recv_decode(1)[0]), runs)
    return t, rx, torch.cat(played[-2:], dim=1).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--packets", type=int, nargs="+", default=[1, 50])
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    N = a.rows
    res = {"runs": a.runs, "rows": N, "frame_samples": 320, "packet_samples": 640, "kernel_source_hash": solo_amd.kernel_source_hash(),
           "shader_clock_mhz_before": solo_amd.shader_clock_mhz(), "shapes": []}
    d, rx, heard = played_rows(torch, N, a.runs)
    res["d_recv_decode_one_packet"] = d
    rooms8 = torch.from_numpy((np.random.default_rng(1).permutation(N) // 8).astype(np.int32)).cuda()
    one_room = torch.zeros((N,), dtype=torch.int32, device="cuda")
    for P in a.packets:
        pcm = heard.repeat(1, (P + 1) // 2, 1)[:, :P].contiguous()              # the played signal, repeated
        v = solo_amd.Vad(N, 320)
        o = v.run(pcm)
        sh = {"packets": P, "a_vad": timed(torch, lambda: v.run(pcm), a.runs)}
        sh["a_vad"]["per_row_packet_us"] = sh["a_vad"]["ms"] * 1e3 / (N * P)
        s = v.select(o["sa"], o["level"], rooms8, n_rooms=N // 8)
        sh["select_count_rooms_of_8"] = v.count(s["count"])
        sh["b_select_rooms_of_8"] = timed(torch, lambda: v.select(o["sa"], o["level"], rooms8, n_rooms=N // 8), a.runs)
        sh["b_select_one_room"] = timed(torch, lambda: v.select(o["sa"], o["level"], one_room, n_rooms=1), a.runs)
        dst = torch.empty_like(pcm)
        sh["c_copy"] = timed(torch, lambda: dst.copy_(pcm), a.runs)
        out = torch.zeros_like(pcm)
        sh["e_mix_rooms_of_8"] = timed(torch, lambda: rx.mix(pcm, rooms8, max_speakers=0, out=out), a.runs)
        sh["a_over_c"] = round(sh["a_vad"]["ms"] / sh["c_copy"]["ms"], 2)
        sh["a_over_d_per_packet"] = round(sh["a_vad"]["ms"] / P / d["ms"], 4)
        sh["a_over_e"] = round(sh["a_vad"]["ms"] / sh["e_mix_rooms_of_8"]["ms"], 3)
        res["shapes"].append(sh)
    rx.close()
    res["shader_clock_mhz_after"] = solo_amd.shader_clock_mhz()
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()

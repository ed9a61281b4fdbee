#!/usr/bin/env python3
"""Cost of the level control stage (solo_agc) at 4096 rows x 1 and x 50 packets of 640 samples, HIP-event medians after a warm-up,
next to its reference points, measured in the same process:

  a  solo_agc                       the C entry point on the caller's buffers, with the VAD's level and activity (and without: the
                                    stage computes the level itself), and solo_amd.Agc.run, which allocates its four outputs
  b  solo_vad                       the same rows: the C entry point on the caller's buffers, and solo_amd.Vad.run
  c  a device copy of the same PCM  the floor of anything that reads and writes the rows once
  d  the tick of INTEGRATION.md section 2, one packet: play-out (solo_recv_decode), solo_vad, solo_agc, solo_vad_select on the levelled
     levels, solo_mix_selected on the levelled rows (rooms of 8, three speakers) -- with the stage, and without it (the selection on the
     VAD's levels, the mix on the played rows)

  python tools/agc_bench.py [--rows 4096] [--packets 1 50] [--runs 9] [--out profiles/agc.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import solo_amd                       # noqa: E402
from vad_bench import timed           # noqa: E402
from solo_amd.synth import synth_stream  # noqa: E402


def receiver(torch, N, packets):
    """N streams encoded and queued, `packets` packets each -> the receiving handle"""
    base = [synth_stream(i, packets) for i in range(64)]
    x = np.stack([base[i % 64] for i in range(N)]).reshape(N, packets, 640)
    tx = solo_amd.SoloBatch(N, rate=13600, encoder=True, decoder=False, slot_bytes=512)
    bits, nb, st = tx.encode(torch.from_numpy(x).cuda())
    rec, pay, cnt = tx.send_pack(bits, nb)
    c = tx.send_count(cnt)
    assert int(st.abs().max()) == 0 and c["refused"] == 0 and c["records"] == c["records_needed"] > 0, c
    tx.close()
    rx = solo_amd.SoloBatch(N, encoder=False, decoder=True)
    rx.recv_create(packets, 256, 0)
    rx.recv_insert(rec[:c["records"]].contiguous(), pay)
    return rx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--packets", type=int, nargs="+", default=[1, 50])
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    N, runs = a.rows, a.runs
    res = {"runs": runs, "rows": N, "frame_samples": 320, "packet_samples": 640, "kernel_source_hash": solo_amd.kernel_source_hash(),
           "shader_clock_mhz_before": solo_amd.shader_clock_mhz(), "shapes": []}
    lib = solo_amd.load_library()
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rooms8 = torch.from_numpy((np.random.default_rng(1).permutation(N) // 8).astype(np.int32)).cuda()
    # d: the tick, one packet per timed call; three receivers with the same queue, one per variant
    ticks = {}
    heard = None
    for name in ("playout_only", "without_agc", "with_agc"):
        rx = receiver(torch, N, runs + 1)
        v, g = solo_amd.Vad(N, 320), solo_amd.Agc(N)
        last = []

        def tick():
            pcm = rx.recv_decode(1)[0]
            last.append(pcm)
            if name == "playout_only":
                return
            o = v.run(pcm)
            level = o["level"]
            if name == "with_agc":
                pcm, level, _, _ = g.run(pcm, level=level, sa=o["sa"], out=pcm)
            s = v.select(o["sa"], level, rooms8, n_rooms=N // 8)
            rx.mix_selected(pcm, rooms8, s["sel"], keep=s["keep"], n_rooms=N // 8)
        ticks[name] = timed(torch, tick, runs)
        if name == "playout_only":
            heard = torch.cat(last[-2:], dim=1).contiguous()
        rx.close()
    res["d_tick_one_packet"] = ticks
    res["d_tick_agc_adds_ms"] = round(ticks["with_agc"]["ms"] - ticks["without_agc"]["ms"], 4)
    prm = solo_amd.solo_agc_params_t(23, 24, 12, 128, 50, 32, 128, 256, 29204, 256)
    for P in a.packets:
        pcm = heard.repeat(1, (P + 1) // 2, 1)[:, :P].contiguous()              # the played signal, repeated
        v, g = solo_amd.Vad(N, 320), solo_amd.Agc(N)
        o = v.run(pcm)
        out = torch.empty_like(pcm)
        lo = torch.empty((N, P), dtype=torch.uint8, device="cuda")
        go = torch.empty((N, P), dtype=torch.int16, device="cuda")
        cnt = torch.zeros((4,), dtype=torch.int32, device="cuda")
        sa, det = torch.empty_like(o["sa"]), None
        agc = lambda level, act: lib.solo_agc(g.h, None, N, pcm.data_ptr(), P, 640, level, act, 2, C.byref(prm), out.data_ptr(), lo.data_ptr(),
                                              go.data_ptr(), cnt.data_ptr(), stream())
        sh = {"packets": P}
        sh["a_agc"] = timed(torch, lambda: agc(o["level"].data_ptr(), o["sa"].data_ptr()), runs)
        sh["a_agc"]["per_row_packet_us"] = sh["a_agc"]["ms"] * 1e3 / (N * P)
        sh["agc_count"] = g.count(cnt)
        sh["a_agc_own_level"] = timed(torch, lambda: agc(None, None), runs)
        sh["a_agc_python"] = timed(torch, lambda: g.run(pcm, level=o["level"], sa=o["sa"], out=out), runs)
        sh["b_vad"] = timed(torch, lambda: lib.solo_vad(v.h, None, N, pcm.data_ptr(), P, 640, sa.data_ptr(), det, lo.data_ptr(), None, stream()), runs)
        sh["b_vad_python"] = timed(torch, lambda: v.run(pcm), runs)
        sh["c_copy"] = timed(torch, lambda: out.copy_(pcm), runs)
        sh["a_over_b"] = round(sh["a_agc"]["ms"] / sh["b_vad"]["ms"], 3)
        sh["a_over_c"] = round(sh["a_agc"]["ms"] / sh["c_copy"]["ms"], 2)
        res["shapes"].append(sh)
    res["shader_clock_mhz_after"] = solo_amd.shader_clock_mhz()
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()

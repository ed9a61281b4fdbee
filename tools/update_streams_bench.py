#!/usr/bin/env python3
"""Cost of solo_batch_update_streams.

  * one update of 1, 512 and 4096 streams of an idle 4096-stream handle: host time of the call (validation, records, launches) and
    device time (HIP events around it on the caller's stream), medians;
  * a 4096-stream tick loop, one packet per call: every tick encodes one packet of every stream and decodes one packet of every stream
    (bits encoded beforehand, so that the two are independent, as a server's outgoing and incoming streams are), with an update of every
    stream before each tick (both directions; the rate alternates between 13600 and 15600 bps from tick to tick) against no update, with
    asynchronous joins off and on; and the same with an update of 128 streams per tick (one launch per direction; the listed streams
    rotate through the handle).  With joins on, a tick's encode may still run when the next tick starts; the update waits for it (as it
    must: the encoder kernels write the whole stream state back when they end), which is the cost to watch.

The library is called directly with the control arrays made beforehand (the Python binding builds them per call).

  python tools/update_streams_bench.py [--streams 4096] [--ticks 50] [--runs 7] [--out profiles/update_streams.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import solo_amd                       # noqa: E402
from solo_amd.synth import synth_stream  # noqa: E402


def _ctrls(n, rate):
    enc, dec = (solo_amd.USER_Ctrl_enc * n)(), (solo_amd.USER_Ctrl_dec * n)()
    for i in range(n):
        enc[i] = solo_amd.default_enc_ctrl(rate)
        dec[i] = solo_amd.default_dec_ctrl()
    return enc, dec


def one_update(torch, N, counts, runs):
    b = solo_amd.SoloBatch(N, encoder=True, decoder=True, slot_bytes=512)
    lib, h, s = b.lib, b.h, b._stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out = []
    for n in counts:
        idx = (C.c_int32 * n)(*range(0, N, N // n)[:n])
        arrs = [_ctrls(n, r) for r in (15600, 13600)]
        host, dev = [], []
        for r in range(runs + 1):
            enc, dec = arrs[r % 2]
            torch.cuda.synchronize()
            ev[0].record()
            t0 = time.perf_counter()
            assert lib.solo_batch_update_streams(h, idx, n, 3, enc, dec, s) == 0
            t1 = time.perf_counter()
            ev[1].record()
            torch.cuda.synchronize()
            if r:
                host.append((t1 - t0) * 1e3)
                dev.append(ev[0].elapsed_time(ev[1]))
        out.append({"streams": n, "host_ms": round(float(np.median(host)), 4), "device_ms": round(float(np.median(dev)), 4),
                    "host_runs_ms": [round(v, 4) for v in host], "device_runs_ms": [round(v, 4) for v in dev]})
        print(json.dumps({k: v for k, v in out[-1].items() if not k.endswith("runs_ms")}), flush=True)
    b.close()
    return out


def tick_loop(torch, N, ticks, runs, async_join, update):
    """ms per tick (median over runs of `ticks` ticks each); update: streams updated before every tick (0: no update)"""
    P = ticks
    base = np.stack([synth_stream(i, P) for i in range(64)]).reshape(64, P, 640)
    pcm = torch.from_numpy(np.ascontiguousarray(base[np.arange(N) % 64])).cuda()
    b = solo_amd.SoloBatch(N, encoder=True, decoder=True, slot_bytes=512)
    bits_in, nb_in, _ = b.encode(pcm)                          # the incoming packets of the loop
    torch.cuda.synchronize()
    b.reset()
    b.set_async_join(async_join)
    lib, h, s = b.lib, b.h, b._stream()
    n = update or 1
    lists = [(C.c_int32 * n)(*sorted((t * n + j) % N for j in range(n))) for t in range(ticks)]
    arrs = [_ctrls(n, r) for r in (13600, 15600)]
    x = [pcm[:, t:t + 1].contiguous() for t in range(ticks)]
    bi = [bits_in[:, t:t + 1].contiguous() for t in range(ticks)]
    ni = [nb_in[:, t:t + 1].contiguous() for t in range(ticks)]
    outs = [(torch.zeros((N, 1, 512), dtype=torch.uint8, device="cuda"), torch.zeros((N, 1, 2), dtype=torch.int16, device="cuda"),
             torch.zeros((N,), dtype=torch.int32, device="cuda")) for _ in range(2)]       # two calls in flight need two sets of outputs
    pcm_out = torch.zeros((N, 1, 640), dtype=torch.int16, device="cuda")
    st_dec = torch.zeros((N,), dtype=torch.int32, device="cuda")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    per_tick = []
    for r in range(runs + 1):
        torch.cuda.synchronize()
        ev[0].record()
        for t in range(ticks):
            if update:
                enc, dec = arrs[t % 2]
                assert lib.solo_batch_update_streams(h, lists[t], n, 3, enc, dec, s) == 0
            o = outs[t % 2]
            assert lib.solo_batch_encode(h, x[t].data_ptr(), 1, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), s) == 0
            assert lib.solo_batch_decode(h, bi[t].data_ptr(), ni[t].data_ptr(), None, 1, pcm_out.data_ptr(), st_dec.data_ptr(), s) == 0
        if async_join:
            b.wait_encode(0)
        ev[1].record()
        torch.cuda.synchronize()
        assert int(outs[0][2].abs().max()) == 0 and int(st_dec.abs().max()) == 0
        if r:
            per_tick.append(ev[0].elapsed_time(ev[1]) / ticks)
    b.close()
    return float(np.median(per_tick)), [round(v, 4) for v in per_tick]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--ticks", type=int, default=50)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    N = a.streams
    res = {"streams": N, "ticks": a.ticks, "runs": a.runs, "kernel_source_hash": solo_amd.kernel_source_hash(),
           "shader_clock_mhz_before": solo_amd.shader_clock_mhz()}
    res["one_update"] = one_update(torch, N, [c for c in (1, 512, 4096) if c <= N], a.runs)
    res["tick_loop"] = []
    for async_join in (False, True):
        counts = [0] + [c for c in (128, N) if c <= N]
        legs = {}
        for update in (counts if async_join is False else counts[::-1]):        # (alternating order)
            legs[update] = tick_loop(torch, N, a.ticks, a.runs, async_join, update)
        for update in counts[1:]:
            c = {"async_join": async_join, "updated_streams_per_tick": update, "no_update_ms_per_tick": round(legs[0][0], 4),
                 "update_every_tick_ms_per_tick": round(legs[update][0], 4), "update_cost_ms_per_tick": round(legs[update][0] - legs[0][0], 4),
                 "ratio": round(legs[update][0] / legs[0][0], 4), "no_update_runs_ms": legs[0][1], "update_runs_ms": legs[update][1]}
            res["tick_loop"].append(c)
            print(json.dumps({k: v for k, v in c.items() if not k.endswith("runs_ms")}), flush=True)
    res["shader_clock_mhz_after"] = solo_amd.shader_clock_mhz()
    txt = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")
    else:
        print(txt)


if __name__ == "__main__":
    main()

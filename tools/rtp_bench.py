#!/usr/bin/env python3
"""Cost of RTP framing and parsing (solo_rtp_pack, solo_rtp_parse) at 4096 streams x 1 packet (a tick) and x 50, 13.6 kbps, next to the
stages on either side of them on the same data, in one run:

  (a) solo_rtp_pack of the records solo_send_pack wrote, with and without the audio-level extension (each into a wire of its own)
  (b) solo_rtp_parse of BOTH wires: datagrams that carry the level extension (X = 1, 20 header bytes, the element walk; every one
      must come back with its level) and datagrams that do not; and of the levels wire without the two optional outputs
  (c) solo_send_pack, the stage in front of (a)
  (d) solo_recv_insert of the arrivals (b) wrote, the stage behind (b) (the ring is emptied before every call; that reset is timed alone
      and taken off)

Every call goes through the C ABI with buffers allocated once (what a server does; the Python methods add argument checks and a count
tensor per call).  Every figure is ms per call: HIP events around `iters` back-to-back calls, `iters` chosen per stage so that a window
lasts about 50 ms, after a warm-up of the same calls; the median over `runs` windows, with the smallest and the largest next to it.
Back-to-back calls measure the larger of the host's enqueue time and the device's time per call: the figures BOUND THE CALL FROM ABOVE
and are not kernel time - at a one-packet tick, three or two launches of a few microseconds each, the host's share may be all of it.
Read (a) and (b) against (c) and (d), which are measured the same way.  The pack's copy is also given as bytes per second: wire bytes
written plus payload bytes read, over the call.

  python tools/rtp_bench.py [--streams 4096] [--packets 1 50] [--runs 9] [--out profiles/rtp.json]
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

WINDOW_MS = 50.0


def timed(torch, fn, runs, warm=5):
    """fn() -> the status of one call"""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def window(iters):
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(iters):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / iters
    for _ in range(warm):
        assert fn() == 0
    iters = int(min(5000, max(10, WINDOW_MS / max(window(10), 1e-4))))
    ms = [window(iters) for _ in range(runs)]
    return {"ms": round(float(np.median(ms)), 5), "min_ms": round(min(ms), 5), "max_ms": round(max(ms), 5), "iters": iters,
            "window_ms": round(float(np.median(ms)) * iters, 1)}


def shape(torch, N, P, runs):
    pcm = torch.from_numpy(np.stack([synth_stream(i % 64, P) for i in range(N)]).reshape(N, P, 640)).cuda()
    tx = solo_amd.SoloBatch(N, rate=13600, encoder=True, decoder=False, slot_bytes=512)
    bits, nb, _ = tx.encode(pcm)
    records, payload, scount = tx.send_pack(bits, nb, first_seq=1000)
    sc = tx.send_count(scount)
    assert sc["records"] == sc["records_needed"] and sc["refused"] == 0
    n, M = sc["records"], records.shape[0]
    rng = np.random.default_rng(1)
    rtp = solo_amd.Rtp(N, 640)
    # (distinct SSRCs all over the 32 bits: an odd multiplier is a bijection mod 2^32)
    rtp.bind(list(range(N)), [(i + 1) * 2654435761 % 2 ** 32 for i in range(N)], [int(v) for v in rng.integers(0, 2 ** 32, N)],
             [int(v) for v in rng.integers(0, 2 ** 16, N)], (96, 97), level_id=1)
    level = torch.from_numpy(rng.integers(0, 128, (N, 64), dtype=np.uint8)).cuda()
    st, L = tx._stream(), tx.lib
    res = {"streams": N, "packets": P, "datagrams": n, "payload_bytes": sc["bytes"]}
    z = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device="cuda")
    cap = sc["bytes"] + 23 * M
    # (a) two wires, two datagram tables: with and without the extension
    out = {}
    for name, lv in (("levels", level), ("plain", None)):
        dgrams, wire, cnt = z((M, 2), torch.int32), z((cap,), torch.uint8), z((8,), torch.int32)
        call = lambda dgrams=dgrams, wire=wire, cnt=cnt, lv=lv: L.solo_rtp_pack(
            rtp.h, records.data_ptr(), scount.data_ptr(), M, payload.data_ptr(), payload.shape[0], None if lv is None else lv.data_ptr(), 64, dgrams.data_ptr(),
            wire.data_ptr(), cap, cnt.data_ptr(), st)
        key = "a_rtp_pack_levels" if lv is not None else "a_rtp_pack"
        res[key] = timed(torch, call, runs)
        c = rtp.pack_count(cnt)
        assert c["dgrams"] == c["dgrams_needed"] == n and c["refused"] == 0, c
        res[key]["wire_bytes"] = c["bytes"]
        res[key]["copy_GBps"] = round((c["bytes"] + sc["bytes"]) / res[key]["ms"] / 1e6, 2)
        out[name] = (dgrams[:n].contiguous(), wire)
    assert res["a_rtp_pack_levels"]["wire_bytes"] > res["a_rtp_pack"]["wire_bytes"]
    # (c)
    scnt2 = z((8,), torch.int32)
    res["c_send_pack"] = timed(torch, lambda: L.solo_send_pack(tx.h, bits.data_ptr(), nb.data_ptr(), None, P, None, 1000, records.data_ptr(), M, payload.data_ptr(),
                                                               payload.shape[0], scnt2.data_ptr(), st), runs)
    assert tx.send_count(scnt2) == sc
    # (b)
    rx = solo_amd.SoloBatch(N, encoder=False, decoder=True)
    depth = 64
    rx.recv_create(depth, 256, 1000)
    arrivals, lv_out, sq_out, pcnt = z((n, 5), torch.int32), z((n,), torch.uint8), z((n,), torch.int16), z((8,), torch.int32)

    def parse(which, outputs):
        dg, wire = out[which]
        return lambda: L.solo_rtp_parse(rtp.h, rx.h, dg.data_ptr(), n, wire.data_ptr(), wire.shape[0], arrivals.data_ptr(), lv_out.data_ptr() if outputs else None,
                                        sq_out.data_ptr() if outputs else None, pcnt.data_ptr(), st)
    for key, which, outputs, want_levels in (("b_rtp_parse_plain", "plain", True, 0), ("b_rtp_parse_levels_no_outputs", "levels", False, n),
                                             ("b_rtp_parse_levels", "levels", True, n)):
        res[key] = timed(torch, parse(which, outputs), runs)
        pc = rtp.parse_count(pcnt)
        assert pc["accepted"] == n and pc["with_level"] == want_levels, (key, pc)
        res[key]["with_level"] = pc["with_level"]
    # every level came back as it was sent (the last parse was the one with outputs, of the levels wire)
    rec = records[:n].long()
    assert bool((lv_out == level[rec[:, 0], rec[:, 1] % 64]).all())
    # (d) the arrivals of the levels wire
    wire = out["levels"][1]

    def reset():
        return L.solo_recv_create(rx.h, depth, 256, 1000, st)

    def insert():
        return reset() or L.solo_recv_insert(rx.h, arrivals.data_ptr(), n, wire.data_ptr(), wire.shape[0], st)
    rst = timed(torch, reset, runs)
    res["d_recv_insert"] = timed(torch, insert, runs)
    for k in ("ms", "min_ms", "max_ms"):
        res["d_recv_insert"][k] = round(res["d_recv_insert"][k] - rst["ms"], 5)
    res["d_recv_insert"]["ring_reset_ms"] = rst["ms"]
    stats = rx.recv_stats()
    assert stats["inserted"] == n and stats["bad"] == 0, stats
    res["ratios"] = {"pack_levels_over_send_pack": round(res["a_rtp_pack_levels"]["ms"] / res["c_send_pack"]["ms"], 3),
                     "parse_levels_over_recv_insert": round(res["b_rtp_parse_levels"]["ms"] / res["d_recv_insert"]["ms"], 3),
                     "parse_levels_over_plain": round(res["b_rtp_parse_levels"]["ms"] / res["b_rtp_parse_plain"]["ms"], 3)}
    rtp.close()
    tx.close()
    rx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--packets", type=int, nargs="+", default=[1, 50])
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    res = {"runs": a.runs, "window_ms_target": WINDOW_MS, "kernel_source_hash": solo_amd.kernel_source_hash(), "shader_clock_mhz_before": solo_amd.shader_clock_mhz(),
           "shapes": []}
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

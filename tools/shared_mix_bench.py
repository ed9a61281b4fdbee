#!/usr/bin/env python3
"""What shared listener mixes save: the bridge tick behind the decoder, 4096 rows at 16 kHz and 13.6 kbps, max_speakers 3, x 1 and x 50
packets, HIP-event medians after a warm-up, on two floors -- rooms of 8, and one room of 4096:

  (a) the personal tick: solo_mix + solo_batch_encode_streams of every row + solo_send_pack_streams
  (b) the shared tick:   solo_mix_shared + the read-back of its 24-byte count + solo_batch_encode_streams of the speakers on the
                         participants' handle and of the shared rooms on a rooms handle, into one table + solo_send_fanout;
                         the two encode calls one after the other on the caller's stream
  (c) the same, with the rooms' encode call on a second stream beside the speakers' (joined by an event before the fan-out): at one
      packet an encode call is a latency chain of about a millisecond however few rows it has, and two of them in a row cost two
  and solo_mix against solo_mix_shared alone.

Every call goes through the C ABI with buffers allocated once, as a server would; the only host synchronisation inside a measured
interval is the count read-back of (b).

  python tools/shared_mix_bench.py [--rows 4096] [--packets 1 50] [--runs 7] [--out profiles/shared_mix.json]
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


def floor(torch, name, N, P, size, runs, K, pcm):
    n_rooms = N // size
    S = 512
    part = solo_amd.SoloBatch(N, rate=13600, encoder=True, decoder=False, slot_bytes=S)           # the participants' handle
    rooms = solo_amd.SoloBatch(n_rooms, rate=13600, encoder=True, decoder=False, slot_bytes=S)    # one slot per room
    lib, st = part.lib, part._stream()
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    room = torch.from_numpy((np.random.default_rng(1).permutation(N) // size).astype(np.int32)).cuda()
    every = torch.arange(N, dtype=torch.int32, device="cuda")
    out, pcm_spk, pcm_room = torch.zeros_like(pcm), torch.zeros_like(pcm), z((n_rooms, P, 640), torch.int16)
    spk_list, spk_rows, room_list, source = z((N,), torch.int32), z((N,), torch.int32), z((n_rooms,), torch.int32), z((N,), torch.int32)
    bits, nb, status = z((N + n_rooms, P, S), torch.uint8), z((N + n_rooms, P, 2), torch.int16), z((N + n_rooms,), torch.int32)
    rec, pay = z((2 * N * P, 5), torch.int32), z((N * P * S,), torch.uint8)
    mcnt, scnt, shcnt = z((4,), torch.int32), z((8,), torch.int32), z((6,), torch.int32)
    host_cnt = torch.zeros((6,), dtype=torch.int32).pin_memory()
    p = lambda x: x.data_ptr()

    def check(r, what):
        if r:
            raise RuntimeError("%s -> %d" % (what, r))

    def mix():
        check(lib.solo_mix(part.h, p(pcm), N, P, p(room), n_rooms, None, K, p(out), None, None, p(mcnt), st), "solo_mix")

    def mix_shared():
        check(lib.solo_mix_shared(part.h, p(pcm), N, P, p(room), n_rooms, None, K, None, None, p(pcm_spk), p(spk_list), p(spk_rows), p(pcm_room),
                                  p(room_list), p(source), None, None, p(shcnt), st), "solo_mix_shared")

    def personal():
        mix()
        check(lib.solo_batch_encode_streams(part.h, p(every), N, p(out), P, p(bits), p(nb), p(status), st), "solo_batch_encode_streams")
        check(lib.solo_send_pack_streams(part.h, p(every), N, p(bits), p(nb), None, P, None, 0, p(rec), rec.shape[0], p(pay), pay.shape[0], p(scnt), st),
              "solo_send_pack_streams")

    seen = {}
    side, joined = torch.cuda.Stream(), torch.cuda.Event()

    def shared(beside=False):
        mix_shared()
        host_cnt.copy_(shcnt, non_blocking=True)
        torch.cuda.current_stream().synchronize()                   # the read-back: the encode calls take their row counts from the host
        ns, nr = int(host_cnt[2]), int(host_cnt[3])
        seen["speakers"], seen["shared"] = ns, nr
        if ns:
            check(lib.solo_batch_encode_streams(part.h, p(spk_list), ns, p(pcm_spk), P, p(bits), p(nb), p(status), st), "solo_batch_encode_streams")
        if nr:                                                      # (the host has just waited for the mix: a second stream may start at once)
            check(lib.solo_batch_encode_streams(rooms.h, p(room_list), nr, p(pcm_room), P, p(bits[N:]), p(nb[N:]), p(status[N:]),
                                                side.cuda_stream if beside else st), "solo_batch_encode_streams (rooms)")
            if beside:
                joined.record(side)
                torch.cuda.current_stream().wait_event(joined)
        check(lib.solo_send_fanout(part.h, p(bits), p(nb), N + n_rooms, p(source), None, N, None, P, None, 0, p(rec), rec.shape[0], p(pay), pay.shape[0],
                                   p(scnt), st), "solo_send_fanout")

    res = {"floor": name, "rooms": n_rooms}
    res["a_personal_tick"] = timed(torch, personal, runs)
    res["personal_send"] = part.send_count(scnt)
    res["b_shared_tick"] = timed(torch, shared, runs)
    res["shared_send"] = part.send_count(scnt)
    res["shared_count"] = part.mix_shared_count(shcnt)
    assert res["shared_count"]["speakers"] == seen["speakers"], res
    res["b_over_a"] = round(res["b_shared_tick"]["ms"] / res["a_personal_tick"]["ms"], 4)
    res["c_shared_tick_two_streams"] = timed(torch, lambda: shared(True), runs)
    res["c_over_a"] = round(res["c_shared_tick_two_streams"]["ms"] / res["a_personal_tick"]["ms"], 4)
    res["solo_mix"] = timed(torch, mix, runs)
    res["solo_mix_shared"] = timed(torch, mix_shared, runs)
    res["mix_shared_over_mix"] = round(res["solo_mix_shared"]["ms"] / res["solo_mix"]["ms"], 4)
    part.close()
    rooms.close()
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
    res = {"runs": a.runs, "rows": a.rows, "max_speakers": a.max_speakers, "kernel_source_hash": solo_amd.kernel_source_hash(),
           "shader_clock_mhz_before": solo_amd.shader_clock_mhz(), "shapes": []}
    for P in a.packets:
        pcm = torch.from_numpy(np.stack([synth_stream(i % 64, P) for i in range(a.rows)]).reshape(a.rows, P, 640)).cuda()
        res["shapes"].append({"packets": P, "floors": [floor(torch, name, a.rows, P, size, a.runs, a.max_speakers, pcm)
                                                      for name, size in (("rooms_of_8", 8), ("one_room", a.rows))]})
    res["shader_clock_mhz_after"] = solo_amd.shader_clock_mhz()
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Cost of the forwarding tick's middle (solo_forward_levels, solo_forward_route) at 4096 rows, K = 3 slots, one packet a tick, next to the
stages on either side of them on the same data, in one run.  Two shapes: 512 rooms of 8 and ONE room of 4096; in both every row sends
its packet (two descriptions: 8192 datagrams a tick) and three rows a room are voiced, selected and forwarded:

  (a) solo_rtp_parse of the tick's datagrams (20 header bytes, the level extension), the stage in front
  (b) solo_forward_levels of the arrivals and level bytes (a) wrote
  (c) solo_vad_select over what (b) wrote (P = 1, frames = 1)
  (d) solo_forward_route of the same arrivals under the selection of (c): 21 504 records (rooms of 8) or 24 570 (one room)
  (e) solo_rtp_pack of the records (d) wrote, out of the receive buffer, with the slot levels: the stage behind

Every call goes through the C ABI with buffers allocated once.  Every figure is ms per call: HIP events around `iters` back-to-back calls,
`iters` chosen per stage so that a window lasts about 50 ms, after a warm-up of the same calls; the median over `runs` windows, with the
smallest and the largest next to it.  Back-to-back calls measure the larger of the host's enqueue time and the device's time per call: the
figures BOUND THE CALL FROM ABOVE and are not kernel time -- solo_forward_route is nine short launches, solo_forward_levels three.  Read (b)
and (d) against (a) and (e), which are measured the same way.  The route repeats the same tick: its slots are held from the first call
on, every later call forwards the same datagrams again (the steady state of a tick without a switch).

  python tools/forward_bench.py [--rows 4096] [--runs 9] [--out profiles/forward.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import solo_amd                       # noqa: E402

WINDOW_MS = 50.0
K = 3


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


def shape(torch, N, room_size, runs):
    rng = np.random.default_rng(room_size)
    n_rooms = N // room_size
    room_np = (np.arange(N) // room_size).astype(np.int32)
    voiced = np.zeros(N, bool)
    for r in range(n_rooms):
        voiced[r * room_size + rng.permutation(room_size)[:K]] = True
    # the senders' side, once: every row's packet as two datagrams with the level extension
    lens = rng.integers(30, 90, (N, 2))
    rec = np.zeros((2 * N, 5), np.int32)
    rec[:, 0], rec[:, 1], rec[:, 2] = np.repeat(np.arange(N), 2), 1000, np.tile([0, 1], N)
    rec[:, 4] = lens.reshape(-1)
    rec[:, 3] = np.concatenate([[0], np.cumsum(rec[:-1, 4])])
    pool = torch.from_numpy(rng.integers(0, 256, int(rec[:, 4].sum()), dtype=np.uint8)).cuda()
    nd = 2 * N
    scount = np.zeros(8, np.int32)
    scount[0] = scount[1] = nd
    ingest = solo_amd.Rtp(N, 640)
    ingest.bind(list(range(N)), [(i + 1) * 2654435761 % 2 ** 32 for i in range(N)], [int(v) for v in rng.integers(0, 2 ** 32, N)],
                [int(v) for v in rng.integers(0, 2 ** 16, N)], (96, 97), level_id=1)
    level = torch.from_numpy(np.where(voiced, 0x80 | 10, 60).astype(np.uint8).reshape(N, 1)).cuda()
    dgrams, wire, cnt = ingest.pack(torch.from_numpy(rec).cuda(), torch.from_numpy(scount).cuda(), pool, level=level)
    assert ingest.pack_count(cnt)["dgrams"] == nd
    perm = torch.from_numpy(rng.permutation(nd)).cuda()
    dgrams = dgrams[perm].contiguous()                      # the network's order
    # the server
    ring = solo_amd.SoloBatch(N, encoder=False, decoder=True)
    ring.recv_create(8, 256, 1000)
    fwd, vad, egress = solo_amd.Forward(N, K), solo_amd.Vad(N, 320), solo_amd.Rtp(N * K, 640)
    egress.bind(list(range(N * K)), [(i + 1) * 2246822519 % 2 ** 32 for i in range(N * K)], 0, 0, (96, 97), level_id=1)
    st, L = fwd._stream(), fwd.lib
    z = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device="cuda")
    room = torch.from_numpy(room_np).cuda()
    arrivals, lv_in, pcnt = z((nd, 5), torch.int32), z((nd,), torch.uint8), z((8,), torch.int32)
    rowinfo, sa, lvl = z((N, 4), torch.int32), z((N,), torch.uint8), z((N,), torch.uint8)
    sel, vcnt = z((N, 1), torch.uint8), z((4,), torch.int32)
    max_records = K * 2 * (room_size - 1) * n_rooms
    records, send_count = z((max_records, 5), torch.int32), z((8,), torch.int32)
    level_fwd, slot_src, fcnt = z((N * K,), torch.uint8), z((n_rooms, K), torch.int32), z((8,), torch.int32)
    dg2, wire2, pcnt2 = z((max_records, 2), torch.int32), z((max_records * 112,), torch.uint8), z((8,), torch.int32)
    prm = solo_amd.solo_vad_select_params_t(K, 128, 64, 0, 6)
    res = {"rows": N, "room_size": room_size, "rooms": n_rooms, "slots": K, "datagrams": nd}
    res["a_rtp_parse"] = timed(torch, lambda: L.solo_rtp_parse(ingest.h, ring.h, dgrams.data_ptr(), nd, wire.data_ptr(), wire.shape[0], arrivals.data_ptr(),
                                                               lv_in.data_ptr(), None, pcnt.data_ptr(), st), runs)
    pc = ingest.parse_count(pcnt)
    assert pc["accepted"] == nd == pc["with_level"], pc
    res["b_forward_levels"] = timed(torch, lambda: L.solo_forward_levels(arrivals.data_ptr(), lv_in.data_ptr(), nd, N, 255, rowinfo.data_ptr(), sa.data_ptr(),
                                                                         lvl.data_ptr(), st), runs)
    assert bool(((sa == 255).cpu() == torch.from_numpy(voiced)).all()) and int(rowinfo[:, 2].min()) == 2
    res["c_vad_select"] = timed(torch, lambda: L.solo_vad_select(vad.h, None, N, sa.data_ptr(), lvl.data_ptr(), 1, 1, room.data_ptr(), n_rooms, C.byref(prm), None,
                                                                 sel.data_ptr(), None, None, None, vcnt.data_ptr(), st), runs)
    assert bool(((sel[:, 0] != 0).cpu() == torch.from_numpy(voiced)).all())
    res["d_forward_route"] = timed(torch, lambda: L.solo_forward_route(fwd.h, arrivals.data_ptr(), nd, rowinfo.data_ptr(), sel.data_ptr(), room.data_ptr(), N, n_rooms,
                                                                       records.data_ptr(), max_records, send_count.data_ptr(), level_fwd.data_ptr(),
                                                                       slot_src.data_ptr(), fcnt.data_ptr(), st), runs)
    fc = fwd.count(fcnt)
    sc = solo_amd.solo_send_count_t.from_buffer_copy(send_count.cpu().numpy().tobytes())
    assert fc["forwarded"] == 2 * K * n_rooms and fc["not_selected"] == nd - fc["forwarded"] and fc["switches"] == 0, fc
    assert sc.records == sc.records_needed == max_records, (sc.records, sc.records_needed, max_records)
    res["d_forward_route"].update(records=int(sc.records), forwarded=fc["forwarded"], record_bytes_written=20 * int(sc.records))
    res["e_rtp_pack"] = timed(torch, lambda: L.solo_rtp_pack(egress.h, records.data_ptr(), send_count.data_ptr(), max_records, wire.data_ptr(), wire.shape[0],
                                                             level_fwd.data_ptr(), 1, dg2.data_ptr(), wire2.data_ptr(), wire2.shape[0], pcnt2.data_ptr(), st), runs)
    c = egress.pack_count(pcnt2)
    assert c["dgrams"] == c["dgrams_needed"] == max_records and c["refused"] == 0, c
    res["e_rtp_pack"]["wire_bytes"] = c["bytes"]
    res["ratios"] = {"levels_over_parse": round(res["b_forward_levels"]["ms"] / res["a_rtp_parse"]["ms"], 3),
                     "route_over_pack": round(res["d_forward_route"]["ms"] / res["e_rtp_pack"]["ms"], 3)}
    for o in (ingest, egress, fwd, ring):
        o.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--room-sizes", type=int, nargs="+", default=[8, 4096])
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    res = {"runs": a.runs, "window_ms_target": WINDOW_MS, "kernel_source_hash": solo_amd.kernel_source_hash(), "shader_clock_mhz_before": solo_amd.shader_clock_mhz(),
           "shapes": []}
    for size in a.room_sizes:
        res["shapes"].append(shape(torch, a.rows, min(size, a.rows), a.runs))
    res["shader_clock_mhz_after"] = solo_amd.shader_clock_mhz()
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()

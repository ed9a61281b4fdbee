#!/usr/bin/env python3
"""What a given selection saves in the bridge tick: solo_mix_selected against solo_mix_shared under the stateless recipe of
INTEGRATION.md section 2 (the gains masked by the selection, max_speakers 3), on the same rows in the same process -- 4096 rows at 16 kHz,
x 1 and x 50 packets, HIP-event medians after a warm-up, on four floors:

  rooms_of_8_one      512 rooms of 8, one selected member each
  rooms_of_8_none     512 rooms of 8, nobody selected
  rooms_of_8_three    512 rooms of 8, three selected members each
  one_room_three      one room of 4096, three selected members

  a  solo_mix_selected                  no d_energy: the energy pass is not launched
  b  solo_mix_selected with d_energy
  c  solo_mix_shared, the recipe        the existing call: the thing to compare against
  d  a device copy of the same PCM      the floor of anything that reads the rows once

and the speakers + shared count of both forms: the number of encodes the tick then pays.  Every call goes through the C ABI with buffers
allocated once, as a server would.

  python tools/selected_mix_bench.py [--rows 4096] [--packets 1 50] [--runs 7] [--out profiles/selected_mix.json]
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


def floor(torch, h, name, N, P, size, picked, runs, pcm, dst):
    n_rooms = N // size
    lib, st = h.lib, h._stream()
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    room_h = (np.random.default_rng(1).permutation(N) // size).astype(np.int32)
    sel_h = np.zeros((N, P), np.uint8)
    for r in range(n_rooms if picked else 0):
        sel_h[np.flatnonzero(room_h == r)[:picked]] = 1
    room, sel = torch.from_numpy(room_h).cuda(), torch.from_numpy(sel_h).cuda()
    masked = torch.from_numpy(np.where(sel_h[:, -1] != 0, 4096, 0).astype(np.int16)).cuda()      # what solo_vad_select hands on as d_gain_out
    keep = z((N,), torch.uint8)
    pcm_spk, pcm_room = torch.zeros_like(pcm), z((n_rooms, P, 640), torch.int16)
    spk_list, spk_rows, room_list, source = z((N,), torch.int32), z((N,), torch.int32), z((n_rooms,), torch.int32), z((N,), torch.int32)
    nsel, energy = z((n_rooms, P), torch.uint8), z((N, P), torch.int64)
    selcnt, shcnt = z((8,), torch.int32), z((6,), torch.int32)
    p = lambda x: x.data_ptr()

    def check(r, what):
        if r:
            raise RuntimeError("%s -> %d" % (what, r))

    def mix_selected(with_energy=False):
        check(lib.solo_mix_selected(h.h, p(pcm), N, P, p(room), n_rooms, None, p(sel), p(keep), None, p(pcm_spk), p(spk_list), p(spk_rows), p(pcm_room),
                                    p(room_list), p(source), p(nsel), p(energy) if with_energy else None, p(selcnt), st), "solo_mix_selected")

    def recipe():
        check(lib.solo_mix_shared(h.h, p(pcm), N, P, p(room), n_rooms, p(masked), 3, p(keep), None, p(pcm_spk), p(spk_list), p(spk_rows), p(pcm_room),
                                  p(room_list), p(source), None, None, p(shcnt), st), "solo_mix_shared")

    res = {"floor": name, "rooms": n_rooms, "selected_per_room": picked}
    res["a_mix_selected"] = timed(torch, mix_selected, runs)
    res["selected_count"] = h.mix_selected_count(selcnt)
    res["b_mix_selected_with_energy"] = timed(torch, lambda: mix_selected(True), runs)
    res["c_mix_shared_recipe"] = timed(torch, recipe, runs)
    res["recipe_count"] = h.mix_shared_count(shcnt)
    res["d_copy"] = timed(torch, lambda: dst.copy_(pcm), runs)
    res["encodes_selected"] = res["selected_count"]["speakers"] + res["selected_count"]["shared"]
    res["encodes_recipe"] = res["recipe_count"]["speakers"] + res["recipe_count"]["shared"]
    assert res["selected_count"]["rows"] == res["recipe_count"]["rows"] == N, res
    res["a_over_c"] = round(res["a_mix_selected"]["ms"] / res["c_mix_shared_recipe"]["ms"], 4)
    res["b_over_c"] = round(res["b_mix_selected_with_energy"]["ms"] / res["c_mix_shared_recipe"]["ms"], 4)
    spread = lambda t: max(t["runs_ms"]) - min(t["runs_ms"])
    res["a_slower_than_c_beyond_spread"] = bool(res["a_mix_selected"]["ms"] - res["c_mix_shared_recipe"]["ms"] >
                                                max(spread(res["a_mix_selected"]), spread(res["c_mix_shared_recipe"])))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--packets", type=int, nargs="+", default=[1, 50])
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    N = a.rows
    res = {"runs": a.runs, "rows": N, "packet_samples": 640, "kernel_source_hash": solo_amd.kernel_source_hash(),
           "shader_clock_mhz_before": solo_amd.shader_clock_mhz(), "shapes": []}
    h = solo_amd.SoloBatch(4, samplerate=16000, framesize_ms=40, encoder=False)      # any handle will do: only its packet geometry is used
    assert h.packet_samples == 640
    for P in a.packets:
        base = [synth_stream(i, P) for i in range(64)]
        pcm = torch.from_numpy(np.stack([base[i % 64] for i in range(N)]).reshape(N, P, 640)).cuda()
        dst = torch.empty_like(pcm)
        res["shapes"].append({"packets": P, "floors": [floor(torch, h, name, N, P, size, picked, a.runs, pcm, dst)
                                                      for name, size, picked in (("rooms_of_8_one", 8, 1), ("rooms_of_8_none", 8, 0),
                                                                                 ("rooms_of_8_three", 8, 3), ("one_room_three", N, 3))]})
    h.close()
    res["shader_clock_mhz_after"] = solo_amd.shader_clock_mhz()
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Cost of moving stream states between handles (solo_batch_export_streams / solo_batch_import_streams) at 4096 streams, 16 kHz, ring
depth 8 x 256-byte slots with every entry holding two 40-byte descriptions, HIP-event medians (per call, over windows of 20 calls back to back) after a warm-up:

  export / import   one call through the binding, n = 1, 64 and 4096 listed streams (spread evenly over the handle), which = 3
                    (encoder + decoder state) and which = 7 (+ receive queue)
  memcpy2d          the yardstick for a strided copy: hipMemcpy2DAsync, one call per section, of the same section bytes per row from a
                    stand-in array of the handle's layout ([N][record bytes]; the binding does not hand out the handle's own
                    pointers) into the same blob (row pitch = blob stride).  It copies rows 0 .. n - 1 (a 2-D copy cannot follow a
                    list), checks nothing and sums nothing.

GB/s counts the section bytes of the n records once (what both have to move); the queue section counts whole slots for the yardstick
and for the kernels alike, although the kernels read only the declared bytes.

  python tools/migrate_bench.py [--streams 4096] [--runs 7] [--out profiles/migrate_streams.json]
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

DEPTH, SLOT, DESC_BYTES = 8, 256, 40


REPS = 20                             # calls per timed window, back to back on the stream: a window is not one launch gap


def timed(torch, fn, runs):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for r in range(runs + 1):                       # (the first run is a warm-up)
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(REPS):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        if r:
            ms.append(ev[0].elapsed_time(ev[1]) / REPS)
    return {"us": round(float(np.median(ms)) * 1e3, 2), "runs_us": [round(x * 1e3, 2) for x in ms]}


def hip_runtime(torch):
    """the HIP runtime that torch has initialised: its streams and pointers mean nothing to another copy"""
    lib = C.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
    lib.hipMemcpy2DAsync.restype = C.c_int
    lib.hipMemcpy2DAsync.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p]
    return lib


def fill_ring(torch, b, N):
    """both descriptions of DEPTH sequence numbers for every stream"""
    n = N * DEPTH * 2
    i = np.arange(n)
    rec = np.stack([i // (DEPTH * 2), (i // 2) % DEPTH, i % 2, i * DESC_BYTES, np.full(n, DESC_BYTES)], axis=1).astype(np.int32)
    pay = np.random.default_rng(1).integers(0, 256, n * DESC_BYTES, dtype=np.uint8)
    b.recv_insert(torch.from_numpy(rec).cuda(), torch.from_numpy(pay).cuda())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "migrate_streams.json"))
    a = ap.parse_args()
    import torch
    N = a.streams
    hip = hip_runtime(torch)
    src, dst = solo_amd.SoloBatch(N), solo_amd.SoloBatch(N)
    for h in (src, dst):
        h.recv_create(DEPTH, SLOT, 0)
    fill_ring(torch, src, N)
    enc_bytes = src.state_bytes("enc") - 64
    dec_bytes = src.state_bytes("dec") - 64                  # (padded to 16: at most 12 bytes more than the record)
    ring_bytes = 2 * DEPTH * SLOT
    res = {"streams": N, "runs": a.runs, "ring": {"depth": DEPTH, "slot_bytes": SLOT, "bytes_per_description": DESC_BYTES},
           "calls_per_window": REPS, "kernel_source_hash": solo_amd.kernel_source_hash(), "shader_clock_mhz_before": solo_amd.shader_clock_mhz(),
           "record_bytes": {"enc": enc_bytes, "dec": dec_bytes, "recv_section": src.state_bytes("recv") - 64}, "cases": []}
    stand_in = {k: torch.zeros((N, v), dtype=torch.uint8, device="cuda") for k, v in (("enc", enc_bytes), ("dec", dec_bytes), ("ring", ring_bytes))}
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for which, name in ((3, "both"), (7, "both+recv")):
        stride = src.state_bytes(name)
        moved = enc_bytes + dec_bytes + (ring_bytes if which & 4 else 0)
        for n in sorted({1, min(64, N), N}):
            idx = np.unique(np.linspace(0, N - 1, n).astype(np.int32))
            lst = torch.from_numpy(idx).cuda()
            blob, cnt = src.export_streams(lst, name)
            assert src.migrate_count(cnt)["streams"] == n
            assert dst.migrate_count(dst.import_streams(lst, blob, name))["streams"] == n
            case = {"which": which, "n": n, "blob_stride": stride, "section_bytes_per_record": moved}
            case["export"] = timed(torch, lambda: src.export_streams(lst, name, blob=blob), a.runs)
            case["import"] = timed(torch, lambda: dst.import_streams(lst, blob, name), a.runs)

            def yard():
                off = 64
                for k, w in (("enc", enc_bytes), ("dec", dec_bytes)) + ((("ring", ring_bytes),) if which & 4 else ()):
                    r = hip.hipMemcpy2DAsync(blob.data_ptr() + off, stride, stand_in[k].data_ptr(), w, w, n, 3, stream())
                    assert r == 0, r
                    off += w
            case["memcpy2d"] = timed(torch, yard, a.runs)
            for k in ("export", "import", "memcpy2d"):
                case[k]["gb_per_s"] = round(n * moved / (case[k]["us"] * 1e-6) / 1e9, 2)
            case["export_over_memcpy2d_bandwidth"] = round(case["export"]["gb_per_s"] / case["memcpy2d"]["gb_per_s"], 3)
            case["import_over_memcpy2d_bandwidth"] = round(case["import"]["gb_per_s"] / case["memcpy2d"]["gb_per_s"], 3)
            res["cases"].append(case)
            print(json.dumps({k: (v if not isinstance(v, dict) else {"us": v["us"], "gb_per_s": v["gb_per_s"]}) for k, v in case.items()}))
    res["shader_clock_mhz_after"] = solo_amd.shader_clock_mhz()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    src.close()
    dst.close()


if __name__ == "__main__":
    main()

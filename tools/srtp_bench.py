#!/usr/bin/env python3
"""Cost of SRTP protection (solo_srtp_protect, solo_srtp_unprotect) at 4096 streams x 1 packet (a tick: 8192 datagrams) and x 50, 13.6 kbps,
tag 10, next to solo_rtp_pack and solo_rtp_parse measured in the same run on the same data:

  (a) solo_rtp_pack (levels, trailer 10) of the records solo_send_pack wrote
  (b) solo_srtp_protect of that wire.  The call works in place, so every timed call is preceded by a device copy that puts the packed
      wire and datagram table back; the copy is timed alone and taken off
  (c) solo_srtp_unprotect of the protected wire, likewise restored before every call (a second call on a decrypted wire would only
      authenticate and reject)
  (d) solo_rtp_parse of the datagrams (c) hands on

Every call goes through the C ABI with buffers allocated once.  Every figure is ms per call: HIP events around `iters` back-to-back
calls, `iters` chosen so that a window lasts about 50 ms, after a warm-up of the same calls; the median over `runs` windows with the
smallest and the largest next to it.  Back-to-back calls measure the larger of the host's enqueue time and the device's time per call:
the figures bound the call from above.  The registers and LDS of the new kernels come from the built library's metadata.

  python tools/srtp_bench.py [--streams 4096] [--packets 1 50] [--runs 9] [--out profiles/srtp.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import solo_amd                       # noqa: E402
from solo_amd.synth import synth_stream  # noqa: E402
from rtp_bench import timed           # noqa: E402

TAG = 10


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
    seq_offset = [int(v) for v in rng.integers(0, 2 ** 15, N)]
    rtp.bind(list(range(N)), [(i + 1) * 2654435761 % 2 ** 32 for i in range(N)], [int(v) for v in rng.integers(0, 2 ** 32, N)], seq_offset, (96, 97), level_id=1)
    rtp.set_trailer(TAG)
    keys = rng.integers(0, 256, (N, solo_amd.SRTP_MASTER_BYTES), dtype=np.uint8)
    # (the receiver starts at the sender's rollover counter: sequence numbers 2000 + offset .. stay below 2^16 + 2^15 here)
    roc = [(seq_offset[i] + 2 * 1000) >> 16 for i in range(N)]
    rtp.set_keys(list(range(N)), tx=keys, rx=keys, rx_roc=roc, tag_bytes=TAG)
    level = torch.from_numpy(rng.integers(0, 128, (N, 64), dtype=np.uint8)).cuda()
    st, L = tx._stream(), tx.lib
    res = {"streams": N, "packets": P, "datagrams": n, "payload_bytes": sc["bytes"], "tag_bytes": TAG}
    z = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device="cuda")
    cap = sc["bytes"] + (23 + TAG) * M
    dgrams, wire, cnt, scnt = z((M, 2), torch.int32), z((cap,), torch.uint8), z((8,), torch.int32), z((8,), torch.int32)
    # (a)
    res["a_rtp_pack"] = timed(torch, lambda: L.solo_rtp_pack(rtp.h, records.data_ptr(), scount.data_ptr(), M, payload.data_ptr(), payload.shape[0], level.data_ptr(), 64,
                                                             dgrams.data_ptr(), wire.data_ptr(), cap, cnt.data_ptr(), st), runs)
    c = rtp.pack_count(cnt)
    assert c["dgrams"] == c["dgrams_needed"] == n and c["refused"] == 0, c
    res["a_rtp_pack"]["wire_bytes"] = c["bytes"]
    packed_dg, packed = dgrams.clone(), wire.clone()

    def restore(dg_from, wire_from):
        def f():
            dgrams.copy_(dg_from)
            wire.copy_(wire_from)
            return 0
        return f

    def less(r, copy):
        for k in ("ms", "min_ms", "max_ms"):
            r[k] = round(r[k] - copy["ms"], 5)
        r["restore_ms"] = copy["ms"]
        return r
    # (b)
    put_packed = restore(packed_dg, packed)
    copy = timed(torch, put_packed, runs)
    res["b_srtp_protect"] = less(timed(torch, lambda: put_packed() or L.solo_srtp_protect(rtp.h, records.data_ptr(), scount.data_ptr(), M, dgrams.data_ptr(), wire.data_ptr(),
                                                                                           cap, scnt.data_ptr(), st), runs), copy)
    pc = rtp.srtp_count(scnt)
    assert pc["ok"] == n and pc["no_key"] == 0 and pc["malformed"] == 0, pc
    prot_dg, prot = dgrams.clone(), wire.clone()
    assert bool((prot_dg[:n, 1] == packed_dg[:n, 1] + TAG).all())
    # (c)
    out = z((M, 2), torch.int32)
    put_prot = restore(prot_dg, prot)
    copy = timed(torch, put_prot, runs)
    res["c_srtp_unprotect"] = less(timed(torch, lambda: put_prot() or L.solo_srtp_unprotect(rtp.h, dgrams.data_ptr(), n, wire.data_ptr(), cap, out.data_ptr(), scnt.data_ptr(),
                                                                                             st), runs), copy)
    uc = rtp.srtp_count(scnt)
    assert uc["ok"] == n, uc
    assert bool((wire[:c["bytes"]] == packed[:c["bytes"]]).sum() >= c["bytes"] - TAG * n) and bool((out[:n] == packed_dg[:n]).all())
    # (d)
    rx = solo_amd.SoloBatch(N, encoder=False, decoder=True)
    rx.recv_create(64, 256, 1000)
    arrivals, lv_out, sq_out, pcnt = z((n, 5), torch.int32), z((n,), torch.uint8), z((n,), torch.int16), z((8,), torch.int32)
    res["d_rtp_parse"] = timed(torch, lambda: L.solo_rtp_parse(rtp.h, rx.h, out.data_ptr(), n, wire.data_ptr(), cap, arrivals.data_ptr(), lv_out.data_ptr(),
                                                               sq_out.data_ptr(), pcnt.data_ptr(), st), runs)
    assert rtp.parse_count(pcnt)["accepted"] == n
    res["ratios"] = {"protect_over_pack": round(res["b_srtp_protect"]["ms"] / res["a_rtp_pack"]["ms"], 3),
                     "unprotect_over_parse": round(res["c_srtp_unprotect"]["ms"] / res["d_rtp_parse"]["ms"], 3)}
    res["ns_per_datagram"] = {"protect": round(1e6 * res["b_srtp_protect"]["ms"] / n, 3), "unprotect": round(1e6 * res["c_srtp_unprotect"]["ms"] / n, 3)}
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
    from kernel_resources import kernel_resources
    seen = kernel_resources(solo_amd.LIB_PATH)
    kernels = {frag: {k: r[k] for k in ("vgpr", "sgpr", "scratch", "lds")} for frag in ("solo_srtp_protect_kernel", "solo_srtp_unprotect_kernel", "solo_srtp_rx_fold_kernel")
               for name, r in seen.items() if frag in name}
    res = {"runs": a.runs, "kernel_source_hash": solo_amd.kernel_source_hash(), "shader_clock_mhz_before": solo_amd.shader_clock_mhz(), "kernels": kernels, "shapes": []}
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

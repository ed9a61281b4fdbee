#!/usr/bin/env python3
"""Cost of the sender's feedback loop (solo_rate_update, solo_batch_update_rates, solo_rate_send_mask) at 4096 streams, next to its
neighbours on the same streams in the same run:

  (a) solo_rtcp_parse of one receiver report per stream (what produces the feedback rows), then solo_rate_update on those rows
  (b) solo_batch_update_rates with every stream changed and with none changed (all values 0), and the host-array
      solo_batch_update_streams of the same 4096 streams with the same rates (128 records a launch: 32 launches)
  (c) solo_rate_send_mask for 1 and for 50 packets a stream, with a sequence base and a caller's mask

Every call goes through the C ABI with buffers allocated once, measured the way tools/rtcp_bench.py measures: HIP events around
back-to-back calls, the median over `runs` windows with the smallest and the largest next to it.  Back-to-back calls measure the larger
of the host's enqueue time and the device's time per call: the figures BOUND THE CALL FROM ABOVE and are not kernel time.  The same
reports are parsed again and again, so from the second call on the controller sees a block that does not advance (`repeated`): another
branch of the rule, the same loads and stores.

  python tools/rate_bench.py [--streams 4096] [--runs 9] [--out profiles/rate.json]
"""
import argparse
import ctypes as C
import json
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import solo_amd                       # noqa: E402
from rtp_bench import timed           # noqa: E402


def measure(torch, N, runs):
    z = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device="cuda")
    rng = np.random.default_rng(1)
    tx = solo_amd.SoloBatch(N, rate=13600, encoder=True, decoder=False, slot_bytes=512)
    st, L = tx._stream(), tx.lib
    ours, theirs = solo_amd.Rtp(N, 640), solo_amd.Rtp(N, 640)
    ssrc = {}
    for r, mul in ((ours, 2654435761), (theirs, 2246822519)):
        ssrc[r] = [(i + 1) * mul % 2 ** 32 for i in range(N)]
        r.bind(list(range(N)), ssrc[r], [int(v) for v in rng.integers(0, 2 ** 32, N)], [int(v) for v in rng.integers(0, 2 ** 16, N)], (96, 97))
    res = {"streams": N}
    # (a) one receiver report with one block per stream: 32 bytes
    now = (0x83AA7E80 << 32) | 0x1234
    mid = (now >> 16) & 0xFFFFFFFF
    wire = b"".join(struct.pack(">BBHIIIIIII", 0x81, 201, 7, ssrc[theirs][i], ssrc[ours][i], ((i * 7) % 64 << 24) | i, 1000 + i, 5, (mid - 0x3000) & 0xFFFFFFFF, 0x1000)
                    for i in range(N))
    dw = torch.from_numpy(np.frombuffer(wire, np.uint8).copy()).cuda()
    dg = torch.from_numpy(np.array([(32 * i, 32) for i in range(N)], np.int32)).cuda()
    rtcp, rate = solo_amd.Rtcp(N), solo_amd.Rate(N)
    fb, qcnt = z((N, 8), torch.int32), z((16,), torch.int32)
    res["a_rtcp_parse"] = timed(torch, lambda: L.solo_rtcp_parse(rtcp.h, theirs.h, ours.h, dg.data_ptr(), N, dw.data_ptr(), dw.shape[0], now, None, fb.data_ptr(),
                                                                 qcnt.data_ptr(), st), runs)
    pc = rtcp.count("parse", qcnt)
    assert pc["accepted"] == N and pc["blocks"] == N, pc
    prm = solo_amd.solo_rate_params_t(6000, 40000, 13600, 200, 5, 26, 13, 0, 250, 2, 3, 0)
    target, mode, rcnt = z((N,), torch.int32), z((N,), torch.uint8), z((16,), torch.int32)
    res["a_rate_update"] = timed(torch, lambda: L.solo_rate_update(rate.h, fb.data_ptr(), C.byref(prm), target.data_ptr(), mode.data_ptr(), rcnt.data_ptr(), st), runs)
    rc = rate.count(rcnt)
    assert rc["rows"] == N and rc["repeated"] == N, rc
    res["a_rate_update"]["last_call"] = rc
    # (b) the decision applied: from device memory, and from host arrays
    rates = [13600 + 200 * (i % 50) for i in range(N)]
    changed, none, acnt = torch.tensor(rates, dtype=torch.int32, device="cuda"), z((N,), torch.int32), z((4,), torch.int32)

    def apply(v):
        return lambda: L.solo_batch_update_rates(tx.h, None, N, v.data_ptr(), acnt.data_ptr(), st)
    res["b_update_rates_all_changed"] = timed(torch, apply(changed), runs)
    assert tx.rates_count(acnt) == dict(applied=N, kept=0, refused=0, listed=N)
    res["b_update_rates_none_changed"] = timed(torch, apply(none), runs)
    assert tx.rates_count(acnt) == dict(applied=0, kept=N, refused=0, listed=N)
    idx = (C.c_int32 * N)(*range(N))
    ctl = (solo_amd.USER_Ctrl_enc * N)()
    for i in range(N):
        ctl[i] = solo_amd.default_enc_ctrl(rate=rates[i])
    res["b_update_streams_host_arrays"] = timed(torch, lambda: L.solo_batch_update_streams(tx.h, idx, N, 1, ctl, None, st), runs)
    # (c) the mode as a send mask
    mode.copy_(torch.from_numpy((np.arange(N) % 3 == 0).astype(np.uint8)))
    base = torch.from_numpy(rng.integers(0, 2 ** 16, N).astype(np.int32)).cuda()
    for P in (1, 50):
        sin, out = torch.full((N, P), 3, dtype=torch.uint8, device="cuda"), z((N, P), torch.uint8)
        res["c_send_mask_%d" % P] = timed(torch, lambda: L.solo_rate_send_mask(mode.data_ptr(), N, None, N, P, base.data_ptr(), 1000, sin.data_ptr(), out.data_ptr(),
                                                                              st), runs)
        assert int(out.min()) >= 1 and int((out != 3).any(dim=1).sum()) == int((mode != 0).sum())
    res["ratios"] = {"update_rates_all_over_update_streams": round(res["b_update_rates_all_changed"]["ms"] / res["b_update_streams_host_arrays"]["ms"], 4),
                     "rate_update_over_rtcp_parse": round(res["a_rate_update"]["ms"] / res["a_rtcp_parse"]["ms"], 3)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    res = {"runs": a.runs, "kernel_source_hash": solo_amd.kernel_source_hash(), "shader_clock_mhz_before": solo_amd.shader_clock_mhz()}
    res.update(measure(torch, a.streams, a.runs))
    res["shader_clock_mhz_after"] = solo_amd.shader_clock_mhz()
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()

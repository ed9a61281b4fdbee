#!/usr/bin/env python3
"""Cost of subset calls (solo_batch_encode_streams, solo_batch_decode_streams, solo_recv_decode_streams): a 4096-slot handle with 25 / 50 /
75 / 100 % of its slots listed, at P = 1 and P = 50 packets per call, for encode, decode and ring play-out.  The yardstick of a subset
of n streams is a plain handle of n streams doing the same work (not n / N of the full call: the quantiser's chain is as long for 2048
streams as for 4096); the 100 % case is compared with the plain call of the 4096-slot handle as well.  HIP-event medians; the order of
the legs alternates so that a drifting clock favours no side.  The library is called directly, with the outputs and the device list made
beforehand: the Python binding's check of `streams=` copies the list to the host, which is not what is measured here.

  python tools/active_streams_bench.py [--slots 4096] [--runs 7] [--out profiles/active_streams.json]
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

FRACS = (0.25, 0.5, 0.75, 1.0)


def _arrivals(streams, seq0, P, n0, n1):
    """both descriptions of packets seq0 .. seq0 + P - 1 of every listed stream, the payload of (stream position k, packet p) at a fixed
    place of the pool -> int32 [n * P * 2, 5]"""
    k, p = np.meshgrid(np.arange(len(streams)), np.arange(P), indexing="ij")
    k, p = k.reshape(-1), p.reshape(-1)
    off = (k * P + p) * 512
    a = np.stack([np.asarray(streams)[k], seq0 + p, np.zeros_like(k), off, n0[k, p] - n1[k, p]], 1)
    b = np.stack([np.asarray(streams)[k], seq0 + p, np.ones_like(k), off + n0[k, p] - n1[k, p], n1[k, p]], 1)
    return np.concatenate([a, b]).astype(np.int32)


class Leg:
    """one handle doing one kind of call, either on all of its streams (streams=None) or on a list"""

    def __init__(self, torch, op, n_handle, rows, pcm, bits, nb, streams):
        self.t, self.op, self.streams, self.calls = torch, op, streams, 0
        self.b = solo_amd.SoloBatch(n_handle, encoder=op == "encode", decoder=op != "encode", slot_bytes=512, use_md_index=1)
        self.pcm = pcm[rows].contiguous()
        self.bits, self.nb = bits[rows].contiguous(), nb[rows].contiguous()
        self.P = pcm.shape[1]
        if op == "ring":
            self.b.recv_create(64, 256, 0)
            hn0, hn1 = self.nb[:, :, 0].cpu().numpy().astype(np.int64), self.nb[:, :, 1].cpu().numpy().astype(np.int64)
            self.hn = (hn0, hn1)
            self.pool = self.bits.reshape(-1)
            self.ids = list(streams) if streams is not None else list(range(n_handle))
        self.map = None if streams is None else torch.tensor(streams, dtype=torch.int32, device="cuda")
        n = self.pcm.shape[0]
        self.bits_out, self.nb_out = torch.zeros_like(self.bits), torch.zeros_like(self.nb)
        self.pcm_out = torch.zeros((n, self.P, 640), dtype=torch.int16, device="cuda")
        self.st = torch.zeros((n,), dtype=torch.int32, device="cuda")

    def once(self, ev0, ev1):
        if self.op == "ring":          # (the arrivals of this call's sequence numbers are filed outside the timed section)
            arr = _arrivals(self.ids, self.calls * self.P, self.P, *self.hn)
            self.b.recv_insert(self.t.from_numpy(arr).cuda(), self.pool)
        lib, h, s, n, P = self.b.lib, self.b.h, self.b._stream(), self.pcm.shape[0], self.P
        m = self.map.data_ptr() if self.map is not None else None
        ev0.record()
        if self.op == "encode":
            a = (self.pcm.data_ptr(), P, self.bits_out.data_ptr(), self.nb_out.data_ptr(), self.st.data_ptr(), s)
            r = lib.solo_batch_encode_streams(h, m, n, *a) if m else lib.solo_batch_encode(h, *a)
        elif self.op == "decode":
            a = (self.bits.data_ptr(), self.nb.data_ptr(), None, P, self.pcm_out.data_ptr(), self.st.data_ptr(), s)
            r = lib.solo_batch_decode_streams(h, m, n, *a) if m else lib.solo_batch_decode(h, *a)
        else:
            a = (P, self.pcm_out.data_ptr(), self.st.data_ptr(), s)
            r = lib.solo_recv_decode_streams(h, m, n, *a) if m else lib.solo_recv_decode(h, *a)
        ev1.record()
        assert r == 0, (self.op, r)
        self.calls += 1

    def close(self):
        self.b.close()


def time_legs(torch, legs, runs):
    """median ms per leg; the legs take turns, one call each, warm-up call first"""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = {k: [] for k in legs}
    for r in range(runs + 1):
        order = list(legs) if r % 2 == 0 else list(reversed(list(legs)))
        for k in order:
            torch.cuda.synchronize()
            legs[k].once(*ev)
            torch.cuda.synchronize()
            if r:
                ms[k].append(ev[0].elapsed_time(ev[1]))
    return {k: float(np.median(v)) for k, v in ms.items()}, {k: [round(x, 3) for x in v] for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=4096)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--packets", default="1,50")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    N = a.slots
    res = {"slots": N, "runs": a.runs, "kernel_source_hash": solo_amd.kernel_source_hash(), "shader_clock_mhz_before": solo_amd.shader_clock_mhz(),
           "cases": []}
    rng = np.random.default_rng(7)
    for P in (int(v) for v in a.packets.split(",")):
        base = np.stack([synth_stream(i, P) for i in range(64)]).reshape(64, P, 640)
        pcm = torch.from_numpy(np.ascontiguousarray(base[np.arange(N) % 64])).cuda()
        enc = solo_amd.SoloBatch(N, encoder=True, decoder=False, slot_bytes=512, use_md_index=1)
        bits, nb, _ = enc.encode(pcm)
        torch.cuda.synchronize()
        enc.close()
        for op in ("encode", "decode", "ring"):
            for frac in FRACS:
                n = int(round(N * frac))
                lst = sorted(rng.choice(N, n, replace=False).tolist()) if n < N else list(range(N))
                # (at 100 % the handle of n streams IS the 4096-slot handle's plain call)
                legs = {"subset": Leg(torch, op, N, lst, pcm, bits, nb, lst), "handle_of_n": Leg(torch, op, n, lst, pcm, bits, nb, None)}
                med, raw = time_legs(torch, legs, a.runs)
                for leg in legs.values():
                    assert int(leg.st.abs().max()) == 0, op
                    leg.close()
                c = {"op": op, "packets": P, "listed": n, "fraction": frac, "subset_ms": round(med["subset"], 4),
                     "handle_of_n_ms": round(med["handle_of_n"], 4), "subset_vs_handle_of_n": round(med["subset"] / med["handle_of_n"], 4), "runs_ms": raw}
                if n == N:
                    c["subset_vs_plain_call"] = c["subset_vs_handle_of_n"]
                res["cases"].append(c)
                print(json.dumps({k: v for k, v in c.items() if k != "runs_ms"}), flush=True)
    res["shader_clock_mhz_after"] = solo_amd.shader_clock_mhz()
    txt = json.dumps(res, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")
    else:
        print(txt)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""A small fixed sequence of library calls whose kernel launches can be counted: two builds of the library that issue the same launches
give the same kernel names and call counts under

  rocprofv3 --kernel-trace --stats -d OUT -- python tools/launch_counts_workload.py

(kernel trace only, no counters; `python tools/summarize_profile.py` or the *_kernel_stats.csv under OUT has the table).  At the 16 kHz
rate and again at 32 kHz, on a handle of 256 streams and 4 packets per call:

  * one encode and one decode with description loss of every stream;
  * one encode and one decode of a listed subset (every third stream);
  * one reset_streams and one update_streams of 200 streams, both directions: more records than one list launch carries (128), so each
    is two launches per direction.

The outputs are not compared with anything (the parity tests do that); the script only fails when a call does.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import solo_amd                          # noqa: E402
from solo_amd.synth import synth_stream  # noqa: E402

N, P, N_CTL = 256, 4, 200


def run(torch, samplerate):
    rate = 13600 if samplerate == 16000 else 24000
    b = solo_amd.SoloBatch(N, rate=rate, encoder=True, decoder=True, slot_bytes=512, samplerate=samplerate)
    k = samplerate // 16000
    x = np.stack([synth_stream(i, P * k) for i in range(N)]).reshape(N, P, b.packet_samples)        # (the generator's 16 kHz signal, read at the handle's rate)
    pcm = torch.from_numpy(x).cuda()
    recv = torch.from_numpy(np.random.default_rng(7).integers(0, 4, size=(N, P), dtype=np.uint8)).cuda()
    bits, nb, st = b.encode(pcm)
    b.decode(bits, nb, recv)
    sub = list(range(0, N, 3))
    sbits, snb, _ = b.encode(pcm[sub].contiguous(), streams=sub)
    b.decode(sbits, snb, recv[sub].contiguous(), streams=sub)
    ctl = list(range(N_CTL))
    b.reset_streams(ctl, rate=rate, use_md_index=0)
    b.update_streams(ctl, rate=rate + 2000, use_md_index=1)
    torch.cuda.synchronize()
    assert int(st.abs().max()) == 0
    b.close()


if __name__ == "__main__":
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    for fs in (16000, 32000):
        run(torch, fs)
    print("launch_counts_workload: done")

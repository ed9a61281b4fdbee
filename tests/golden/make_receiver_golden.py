#!/usr/bin/env python3
"""Regenerates tests/golden/receiver_split.npz from the COMPILED reference (oracle/_ref, fixed-point tree): the three scenarios of
tests/test_gpu_receiver.py (24 streams x 10 packets; useMDIndex 0 / 1 at 16 kHz, useMDIndex 1 at 32 kHz), encoded by the reference
encoder and decoded by the reference decoder fed the correctly ordered (ptr, nBytes, lostflag) call under the test's arrival mask.
Per scenario `m<mdi>_<fs>`: nb_* int16 [24, 10, 2] = nBytesOut, pcrc_* uint32 [24, 10] = CRC-32 of every payload,
crc_* uint32 [24, 10] = CRC-32 of every decoded packet.  Data only; runs where /root/reference was available to build oracle/_ref."""
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import refcodec as R  # noqa: E402
import solo_testlib as T  # noqa: E402

N, P = 24, 10
CASES = [(0, 16000), (1, 16000), (1, 32000)]       # (useMDIndex, samplerate) as parametrised in the test


def scenario(mdi, fs):
    pcm = np.stack([(R.synth_stream if fs == 16000 else T.synth_stream_32k)(300 + i, P) for i in range(N)])
    recv = T.bernoulli_recv(N, P, 0.3, 11 + mdi)
    nb = np.zeros((N, P, 2), np.int16)
    pcrc = np.zeros((N, P), np.uint32)
    crc = np.zeros((N, P), np.uint32)
    for i in range(N):
        e = R.RefEncoder("fix", rate=13600 if fs == 16000 else 24000, use_md_index=mdi, samplerate=fs)
        d = R.RefDecoder("fix", use_md_index=mdi, samplerate=fs)
        for p in range(P):
            pl, n0, n1 = e.encode(pcm[i, p])
            nb[i, p] = (n0, n1)
            pcrc[i, p] = zlib.crc32(pl[:n0])
            m = int(recv[i, p])
            out, ret = d.decode(*R.map_loss(pl[:n0], n0, n1, not (m & 1), not (m & 2)))
            assert ret == 0
            crc[i, p] = zlib.crc32(out.tobytes())
        e.close()
        d.close()
    return nb, pcrc, crc


def main():
    assert R.have_ref("fix"), "oracle/_ref not built"
    out = {}
    for mdi, fs in CASES:
        k = "m%d_%d" % (mdi, fs)
        out["nb_" + k], out["pcrc_" + k], out["crc_" + k] = scenario(mdi, fs)
    path = os.path.join(HERE, "receiver_split.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()

"""Whole-encoder streams that reach lines of the kernel headers no other input of the suite reaches (tests/golden/rare_branches.npz, found
by tools/debug/rare_branch_search.py in the host emulation built with --coverage), through the host emulation: the reference's payloads
byte for byte, the reference's decode under the fixture's loss mask CRC for CRC; where oracle/_ref is present, the live reference as well.
The file may hold no stream: the search then found none, and profiles/emu_coverage.txt says what it spent."""
import zlib

import numpy as np
import pytest

import refcodec as R
import solo_testlib as T

Z = np.load(T.GOLDEN + "/rare_branches.npz")
N = int(Z["n_streams"])


def stream(i):
    k = "s%02d_" % i
    wb, rate, joint, mdi = (int(v) for v in Z[k + "cfg"])
    return dict(wb=wb, rate=rate, joint=joint, mdi=mdi), {f: Z[k + f] for f in ("pcm", "recv", "bits", "nbytes", "dec_crc", "dec_ret")}


def test_fixture_shape():
    assert 0 <= N <= 32
    for i in range(N):
        cfg, s = stream(i)
        assert s["pcm"].shape == (s["recv"].shape[0], 1280 if cfg["wb"] else 640) and s["pcm"].shape[0] <= 12 and s["recv"][0] == 3
        assert (s["nbytes"][:, 0] > 0).all() and str(Z["s%02d_what" % i])


def _through(enc, dec, cfg, s):
    for p in range(s["pcm"].shape[0]):
        pl, n0, n1 = enc.encode(s["pcm"][p])
        assert (n0, n1) == tuple(int(v) for v in s["nbytes"][p]) and pl == s["bits"][p, :n0].tobytes(), p
        m = int(s["recv"][p])
        x, ret = dec.decode(pl, n0, n1, 1) if m == 0 else dec.decode(*R.map_loss(pl, n0, n1, not (m & 1), not (m & 2)))
        assert ret == int(s["dec_ret"][p]) and zlib.crc32(x.tobytes()) == int(s["dec_crc"][p]), p


def test_emulation():
    for i in range(N):
        cfg, s = stream(i)
        flags = cfg["mdi"] | (2 if cfg["joint"] else 0)
        _through(T.EmuEncoder(cfg["rate"], flags, wb=bool(cfg["wb"])), T.EmuDecoder(flags & 3, wb=bool(cfg["wb"])), cfg, s)


@pytest.mark.skipif(not R.have_ref("fix"), reason="oracle/_ref not built")
def test_live_reference():
    for i in range(N):
        cfg, s = stream(i)
        sr = 32000 if cfg["wb"] else 16000
        _through(R.RefEncoder("fix", rate=cfg["rate"], joint=cfg["joint"], dtx=0, use_md_index=cfg["mdi"], samplerate=sr),
                 R.RefDecoder("fix", joint=cfg["joint"], use_md_index=cfg["mdi"], samplerate=sr), cfg, s)

"""Whole-encoder streams that reach lines of the kernel headers no other input of the suite reaches (tests/golden/rare_branches.npz, see
tests/test_rare_branches_reference.py), on the GPU through SoloBatch, grouped by configuration: the reference's payloads byte for byte, the
decode under the fixture's loss mask CRC for CRC.  These run the PRODUCT kernels' own copies of the stage functions, which the
function-level probe (tests/test_gpu_fn_probe.py) cannot."""
import zlib

import numpy as np
import pytest

import solo_testlib as T

pytestmark = pytest.mark.gpu

Z = np.load(T.GOLDEN + "/rare_branches.npz")
N = int(Z["n_streams"])
GROUPS = {}
for _i in range(N):
    GROUPS.setdefault(tuple(int(v) for v in Z["s%02d_cfg" % _i]), []).append(_i)


def test_fixture_is_grouped():
    assert sum(len(v) for v in GROUPS.values()) == N <= 32


def test_streams_by_configuration():
    for cfg in sorted(GROUPS):
        _configuration(cfg)


def _configuration(cfg):
    import torch
    import solo_amd
    wb, rate, joint, mdi = cfg
    ids = GROUPS[cfg]
    pcm = np.stack([Z["s%02d_pcm" % i] for i in ids])
    recv = np.stack([Z["s%02d_recv" % i] for i in ids])
    b = solo_amd.SoloBatch(len(ids), rate=rate, encoder=True, decoder=True, slot_bytes=512, use_md_index=mdi, joint=joint, samplerate=32000 if wb else 16000)
    bits, nb, st = b.encode(torch.from_numpy(pcm).to(b.device))
    assert int(st.abs().max()) == 0
    hb, hn = bits.cpu().numpy(), nb.cpu().numpy()
    for k, i in enumerate(ids):
        want_nb, want = Z["s%02d_nbytes" % i], Z["s%02d_bits" % i]
        assert np.array_equal(hn[k], want_nb), (i, str(Z["s%02d_what" % i]))
        for p in range(pcm.shape[1]):
            n = int(want_nb[p, 0])
            assert np.array_equal(hb[k, p, :n], want[p, :n]), (i, p, str(Z["s%02d_what" % i]))
    out, st2 = b.decode(bits, nb, torch.from_numpy(recv).to(b.device))
    assert int(st2.abs().max()) == 0          # (the fixture keeps streams whose every packet the reference decodes with status 0)
    ho = out.cpu().numpy()
    for k, i in enumerate(ids):
        for p in range(pcm.shape[1]):
            assert zlib.crc32(ho[k, p].tobytes()) == int(Z["s%02d_dec_crc" % i][p]), (i, p, int(recv[k, p]))

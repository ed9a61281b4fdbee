"""CPU companion of tests/test_gpu_burg_sites.py: the compiled reference encodes every input family (each packet with a positive length,
the status the parity tests rely on) and writes exactly the recorded fixture; the families are what their names say."""
import numpy as np
import pytest

import burg_sites_inputs as B
import refcodec as R
import solo_testlib as T


def test_families_are_distinct_streams_of_the_stated_shape():
    for name in B.FAMILIES + (B.WB,):
        x = B.family(name)
        assert x.dtype == np.int16 and x.shape == (B.N, B.P, 1280 if name == B.WB else 640), name
        assert len({x[i].tobytes() for i in range(B.N)}) == B.N, name
    assert not B.family("silence_then_full_scale")[:, :2].any() and np.abs(B.family("silence_then_full_scale")[:, 3:].astype(np.int32)).max() > 32000
    assert np.abs(B.family("lsb_noise")).max() == 1 and np.abs(B.family("silence")).max() == 1
    for name in ("sinusoid", "two_tone"):                      # - 6 dBFS
        assert 16000 <= np.abs(B.family(name).astype(np.int32)).max() <= 16384, name


def test_fixture_holds_every_family():
    z = np.load(T.GOLDEN + "/burg_sites.npz")
    for name in B.FAMILIES + (B.WB,):
        assert z[name + "/bits"].shape == (B.N, B.P, B.SLOT) and z[name + "/nbytes"].shape == (B.N, B.P, 2), name
        assert (z[name + "/nbytes"][:, :, 0] > 0).all(), name


@pytest.mark.skipif(not R.have_ref("fix"), reason="oracle/_ref not built")
@pytest.mark.parametrize("name", B.FAMILIES + (B.WB,))
def test_reference_encodes_the_family_and_matches_the_fixture(name):
    z = np.load(T.GOLDEN + "/burg_sites.npz")
    bits, nb = B.reference(name)                               # asserts the status of every packet
    assert np.array_equal(nb, z[name + "/nbytes"]) and np.array_equal(bits, z[name + "/bits"])

"""CPU companion of tests/test_gpu_dot_sites.py: the compiled reference encodes every input family (each packet with a positive length
within the slot, the status the parity tests rely on) and writes exactly the recorded fixture; the families are what their names say; the
host build of the kernel source, whose packed sums are the host twins of the device's, reproduces the fixture on a sample of streams."""
import numpy as np
import pytest

import dot_sites_inputs as B
import refcodec as R
import solo_testlib as T


def test_families_are_distinct_streams_of_the_stated_shape():
    for name in B.FAMILIES + (B.WB,):
        x = B.family(name)
        assert x.dtype == np.int16 and x.shape == (B.N, B.P, 1280 if name == B.WB else 640), name
        assert len({x[i].tobytes() for i in range(B.N)}) == B.N, name
    s = B.family("silence_then_full_scale").reshape(B.N, -1)
    onset = np.array([int(np.flatnonzero(s[i])[0]) for i in range(B.N)])
    assert (onset >= 2 * 640).all() and (onset < 3 * 640).all() and {int(v) & 1 for v in onset} == {0, 1}
    assert np.abs(s[:, 3 * 640:].astype(np.int32)).max() > 32000
    assert np.abs(B.family("lsb_noise")).max() == 1 and np.abs(B.family("silence")).max() == 1
    for name in ("square_full_scale", "alternating_full_scale", "white_full_scale"):
        x = B.family(name)
        assert x.min() == -32768 and x.max() >= 32000, name
    assert set(np.unique(B.family("square_full_scale"))) == {-32768, 32767}


def test_fixture_holds_every_family():
    z = np.load(T.GOLDEN + "/dot_sites.npz")
    for name in B.FAMILIES + (B.WB,):
        assert z[name + "/bits"].shape == (B.N, B.P, B.SLOT) and z[name + "/nbytes"].shape == (B.N, B.P, 2), name
        assert (z[name + "/nbytes"][:, :, 0] > 0).all() and (z[name + "/nbytes"][:, :, 0] <= B.SLOT).all(), name


@pytest.mark.parametrize("name", B.FAMILIES + (B.WB,))
def test_host_build_reproduces_the_fixture(name):
    """every eighth stream through the host emulation of the kernel source (the 32 kHz family through its 32 kHz-mode build)"""
    emu = T.load_emu_wb() if name == B.WB else T.load_emu()
    z = np.load(T.GOLDEN + "/dot_sites.npz")
    pcm = B.family(name)
    for s in range(0, B.N, 8):
        h = emu.emu_enc_create(B.ctor(name)["rate"], 0)
        for p in range(B.P):
            bits, nb = np.zeros(1100, np.uint8), np.zeros(2, np.int16)
            x = np.ascontiguousarray(pcm[s, p])
            n = emu.emu_enc_packet(h, x.ctypes.data, bits.ctypes.data, 1024, nb.ctypes.data)
            assert (int(nb[0]), int(nb[1])) == tuple(int(v) for v in z[name + "/nbytes"][s, p]) and n == nb[0], (name, s, p)
            assert np.array_equal(bits[:n], z[name + "/bits"][s, p, :n]), (name, s, p)
        emu.emu_enc_destroy(h)


@pytest.mark.skipif(not R.have_ref("fix"), reason="oracle/_ref not built")
@pytest.mark.parametrize("name", B.FAMILIES + (B.WB,))
def test_reference_encodes_the_family_and_matches_the_fixture(name):
    z = np.load(T.GOLDEN + "/dot_sites.npz")
    bits, nb = B.reference(name)                               # asserts the status of every packet
    assert np.array_equal(nb, z[name + "/nbytes"]) and np.array_equal(bits, z[name + "/bits"])

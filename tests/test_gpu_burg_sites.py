"""The Burg recursion at its three GPU call sites (whole frame, second half, high band; sx_burg_modified, solo_enc_analysis.h) on inputs
that reach each of its branches: payload bytes and lengths of 64 streams x 6 packets per family against the compiled reference -- live
through oracle/refcodec.py where oracle/_ref is present, and always against its recorded output (tests/golden/burg_sites.npz, written
by tests/golden/make_burg_sites_golden.py), so no family is ever skipped.  Every stream starts from a reset: packet 0 is the first
packet after one (no interpolation, no second-half run).

Which families reach which branch was counted on the host build (SX_NLANES == 1) with -DSX_BURG_COUNT (tools/debug/burg_branches.py;
the full table is in profiles/burg_steps.txt, section 4).  Runs of the recursion out of 768 whole-frame, 704 second-half and 768 high-band
runs per family:
  the hi = false recursion (rshifts <= -2) is what the two low-band sites mostly run, since their input is the gain-scaled residual: every
  run of silence, lsb_noise, white_full_scale, speech_like, silence_then_full_scale and nyquist_full_scale, and 432 + 661 (square_full_scale),
  405 + 404 (sinusoid), 600 + 610 (two_tone) runs.  At the high-band site: every run of silence, lsb_noise, sinusoid and two_tone, 752 of
  speech_like, 260 of silence_then_full_scale;
  the hi = true recursion: low band 336 + 43 (square_full_scale), 363 + 300 (sinusoid), 168 + 94 (two_tone) runs; high band every run of
  white_full_scale, square_full_scale and nyquist_full_scale, 508 of silence_then_full_scale, 16 of speech_like;
  the |num| >= den exit before the last order: 457 high-band runs of nyquist_full_scale (a family added for it) and no other run.  The
  sinusoid and the two-tone signal do NOT reach it at any site -- the conditioning term (WhiteNoiseFrac) keeps |num| < den through all
  orders -- and no input tried reached it at the two low-band sites;
  the two runs of one frame accumulating their first rows differently (64-bit against wrapping 32-bit): 18 second-half runs of
  square_full_scale, 87 of two_tone, 1 of sinusoid; none of silence_then_full_scale, whose low-band runs all have rshifts <= 0."""
import functools

import numpy as np
import pytest

import burg_sites_inputs as B
import refcodec as R
import solo_testlib as T

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _golden():
    return np.load(T.GOLDEN + "/burg_sites.npz")


def _gpu(name):
    import torch
    import solo_amd
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    pcm = B.family(name)
    b = solo_amd.SoloBatch(B.N, encoder=True, decoder=False, slot_bytes=B.SLOT, **B.ctor(name))
    bits, nb, st = b.encode(torch.from_numpy(pcm).cuda())
    torch.cuda.synchronize()
    assert int(st.abs().max()) == 0
    return bits.cpu().numpy(), nb.cpu().numpy()


def _check(name):
    bits, nb = _gpu(name)
    refs = [(_golden()[name + "/bits"], _golden()[name + "/nbytes"])]
    if R.have_ref("fix"):
        refs.append(B.reference(name))
    for rb, rn in refs:
        assert np.array_equal(nb, rn), (name, np.argwhere(nb != rn)[:8])
        assert (rn[:, :, 0] > 0).all()
        for i in range(B.N):
            for p in range(B.P):
                n0 = int(rn[i, p, 0])
                assert np.array_equal(bits[i, p, :n0], rb[i, p, :n0]), (name, i, p)


@pytest.mark.parametrize("name", B.FAMILIES)
def test_family_matches_the_reference_in_every_byte(name):
    """13.6 kbps, 16 kHz API rate: the register-resident recursion"""
    _check(name)


def test_wide_band_build_keeps_the_lds_form():
    """24 kbps, samplerate = 32000: the order-16 analysis takes the LDS form of the recursion, which this file's subject left alone"""
    _check(B.WB)

"""The sites of the analysis and coding kernels that sum products of 16-bit samples two at a time (sx_dot2 / sx_pair / sx_fir_dot2 /
sx_corr_dot2, solo_fix.h): pitch stages 1 and 2 (sx_pitch_analysis_core), the whitening filter of sx_find_pitch_lags, the two filters
of sx_residual_energy, the four whitening filters of the interpolation search (sx_find_LPC) and the first row of the Burg correlations
(sx_burg_modified, all three call sites).  Payload bytes and lengths of 64 streams x 6 packets per family against the compiled
reference -- live through oracle/refcodec.py where oracle/_ref is present, and always against its recorded output
(tests/golden/dot_sites.npz, written by tests/golden/make_dot_sites_golden.py), so no family is ever skipped.  Every stream starts from
a reset.

What the families reach was counted on the host build (SX_NLANES == 1) with -DSX_DOT_COUNT (tools/debug/dot_branches.py; the table is in
profiles/dot_sites.txt, section 4).  Over the eight 16 kHz families, 768 frames each (64 streams x 6 packets x 2 frames):
  lags of both parities at both pitch stages: stage 1 scores every lag 8 .. 72 for both targets of every frame (50 688 even, 49 152 odd
    (target, lag) pairs a family); stage 2 scored 22 068 even and as many odd candidate lags in voiced_harmonic (speech_like: 25 700 each),
    none in silence and lsb_noise, which leave after stage 1; the WINNING 8 kHz lag was even in 248 and odd in 500 frames of
    voiced_harmonic (speech_like: 296 / 406, square_full_scale: 190 / 431, alternating_full_scale: 344 / 187);
  a scaling shift > 0 of the 4 kHz / the 8 kHz signal: 768 / 331 frames of white_full_scale, 768 / 654 of square_full_scale, 768 / 552 of
    alternating_full_scale, 733 / 711 of speech_like, 768 / 767 of voiced_harmonic, 466 / 157 of silence_then_full_scale, none of silence
    and lsb_noise;
  the voiced and the unvoiced branch: voiced / unvoiced frames 748 / 20 (voiced_harmonic), 702 / 66 (speech_like), 621 / 147
    (square_full_scale), 531 / 237 (alternating_full_scale); silence and the noise families are unvoiced throughout (one voiced frame in
    silence_then_full_scale);
  the interpolation search: 704 of 768 frames of every family (all but the first frame of a stream)."""
import functools

import numpy as np
import pytest

import dot_sites_inputs as B
import refcodec as R
import solo_testlib as T

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _golden():
    return np.load(T.GOLDEN + "/dot_sites.npz")


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
    """13.6 kbps, 16 kHz API rate"""
    _check(name)


def test_wide_band_build_matches_the_reference_in_every_byte():
    """24 kbps, samplerate = 32000: order-16 filters (eight pairs a tap loop), the LDS form of the Burg recursion behind the packed first
    row, and the third pitch stage, which was left as it was"""
    _check(B.WB)

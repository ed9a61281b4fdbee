"""The 64-lane device bodies of the LPC / NLSF stage functions on the GPU, one call per case (probe: solo_debug_fn, in a translation unit of
its own, solo_amd/csrc/solo_fn_probe.hip), against the fixture tests/golden/fn_cases*.npz = the compiled reference's outputs, word for
word; where oracle/_ref travelled, against the live reference as well.  One launch per group and call site, one wavefront per case.

Many stage functions have a second body that only the gfx950 build compiles: the root scan of sx_a2nlsf over wave ballots with one root
per lane, the bitonic survivor selection of sx_nlsf_msvq_encode, the row form sx_row_nlsf2a_stable_n with its fall-back to the serial
form, the register-resident Burg recursion.  The host emulation (tests/test_fn_probe_reference.py) compiles the other body, and the
whole-encoder fixtures never reach these functions' rare branches: bandwidth-expansion retries, the fall-back vector and a first root
at 0 in A2NLSF, equal keys at the survivor cut, NLSF vectors that need the reference's corrections, the Burg recursion's early exit and
its clamp of the scaling.  The families of tests/fn_probe_lib.py reach them (their conditions are asserted on the CPU).

What this shows and what not: the probe runs each function's device body as compiled for the PROBE's call.  The product kernels hold
their own copies, specialised for their callers; those are reached by whole-encoder inputs only."""
import numpy as np
import pytest

import fn_probe_lib as F

pytestmark = pytest.mark.gpu

BUILDS = {"nb": F.Build(False), "wb": F.Build(True)}
CASES = [(b, g) for b in BUILDS for g in BUILDS[b].groups]
SENTINEL = 0x5A5AA5A5


def _run(build, unit, site, recs):
    import torch
    import solo_amd
    ow = build.words(unit)[1]
    d_in = torch.from_numpy(np.ascontiguousarray(recs, np.int32)).cuda()
    d_out = torch.full((len(recs) + 1, ow), SENTINEL, dtype=torch.int32, device="cuda")      # (a guard record behind the output)
    solo_amd.debug_fn(build.samplerate, F.fn_id(unit, site), d_in, d_out[:len(recs)])
    got = d_out.cpu().numpy()
    assert (got[len(recs)] == SENTINEL).all(), "the probe wrote behind its output"
    return got[:len(recs)]


@pytest.mark.parametrize("b,group", CASES)
def test_device_body_equals_reference(b, group):
    import refcodec as R
    build = BUILDS[b]
    unit, sites, d = build.groups[group]
    cases = F.load_cases(build, group)
    fams = list(cases)
    recs = np.concatenate([cases[f][0] for f in fams])
    want = np.concatenate([cases[f][1] for f in fams])
    fam_of = np.concatenate([np.full(len(cases[f][0]), k) for k, f in enumerate(fams)])
    assert len(recs) <= 4096
    if R.have_ref("fix"):               # the live reference, where it travelled
        live, _ = F.run_ref(build, group, recs, "fix", fork=False)
        assert np.array_equal(live, want), "the live reference is not the fixture's"
    for site in sites:
        got = _run(build, unit, site, recs)
        bad = np.nonzero((got != want).any(axis=1))[0]
        print("%s %s site %d: %d cases, %d differ" % (b, group, site, len(recs), len(bad)))
        assert len(bad) == 0, "%s site %d: %d of %d cases differ (families %s), first %d (%s): in %s got %s want %s" % (
            group, site, len(bad), len(recs), sorted({fams[k] for k in fam_of[bad]}), bad[0], fams[fam_of[bad[0]]],
            recs[bad[0]][:52].tolist(), got[bad[0]].tolist(), want[bad[0]].tolist())
    if unit == F.NLSF2A:
        # (compared above as word 16: the row form declined exactly where the reference corrects -- its limiter or an unstable filter --
        # and accepted everywhere else)
        assert 0 < int(want[:, 16].sum()) < len(want)


@pytest.mark.parametrize("b", list(BUILDS))
def test_probe_refuses(b):
    import torch
    import solo_amd
    build = BUILDS[b]
    for unit, word, value in ((F.NLSF2A, 3, -1), (F.NLSF2A, 0, 32768), (F.MSVQ, 48, 2), (F.FIND_LPC, build.X + 2, 40000)):
        rec = np.zeros((2, build.words(unit)[0]), np.int32)
        rec[1, word] = value
        got = _run(build, unit, 0, rec)
        assert (got[1] == F.REFUSED).all() and not (got[0] == F.REFUSED).any(), (unit, got)
    iw, ow = build.words(F.A2NLSF)
    d_in, d_out = torch.zeros((1, iw), dtype=torch.int32, device="cuda"), torch.zeros((1, ow + 1), dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):
        solo_amd.debug_fn(build.samplerate, F.fn_id(F.A2NLSF, 0), d_in, d_out)          # not the fn's record size
    with pytest.raises(ValueError):
        solo_amd.debug_fn(build.samplerate, F.fn_id(F.A2NLSF, 3), d_in, d_out[:, :ow].contiguous())
    with pytest.raises(ValueError):
        solo_amd.debug_fn(build.samplerate, 0, d_in.cpu(), d_out)

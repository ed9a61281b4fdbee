"""The function-level probe of the LPC / NLSF stage functions on the CPU (solo_amd/csrc/solo_fn_probe.h, tests/fn_probe_lib.py): the host
emulation's emu_fn against the fixture tests/golden/fn_cases*.npz (the compiled reference's outputs) word for word, the conditions every
family of cases is there for -- from the reference's outputs and plain restatements, so that a family cannot quietly stop reaching its
branch -- and, where oracle/_ref is present, the live reference against the fixture.

The emulation compiles the one-lane body of every stage function; the 64-lane bodies of the gfx950 build run the same cases in
tests/test_gpu_fn_probe.py.

Arms that no family reaches, with the search spent on them (tests/golden/make_fn_cases.py prints the counts):
  * the saturation after ten limiter rounds of NLSF2A (solo_common.h, `if (i == 10)`): 0 of 24 000 non-decreasing vectors per order;
  * the |num| >= den exit of the Burg recursion at the second-half site of the 16 kHz build (2 x 50 samples): 0 of the 1 280 fixture
    records (full-scale alternations, DC, square waves of every period, periodic blocks and impulses over the whole range of levels);
  * the negative first energy shift of sx_find_LPC: 0 of 1 760 records per build, asserted to stay 0 with the reason."""
import ctypes as C

import numpy as np
import pytest

import fn_probe_lib as F

BUILDS = {"nb": F.Build(False), "wb": F.Build(True)}
CASES = [(b, g) for b in BUILDS for g in BUILDS[b].groups]


def _count(flags):
    return int(np.sum(np.asarray(flags, bool)))


@pytest.mark.parametrize("b,group", CASES)
def test_emu_equals_fixture(b, group):
    build = BUILDS[b]
    unit, sites, d = build.groups[group]
    cmp_words = 16 if unit == F.NLSF2A else build.words(unit)[1]        # (the emulation has no row form: its `declined` word is -1)
    for fam, (recs, want) in F.load_cases(build, group).items():
        for site in sites:
            got = F.run_emu(build, group, recs, site)
            bad = np.nonzero((got[:, :cmp_words] != want[:, :cmp_words]).any(axis=1))[0]
            assert len(bad) == 0, "%s %s site %d: %d of %d cases differ, first %d: got %s want %s" % (
                group, fam, site, len(bad), len(recs), bad[0], got[bad[0]].tolist(), want[bad[0]].tolist())
            if unit == F.NLSF2A:
                assert (got[:, 16] == -1).all()


@pytest.mark.parametrize("b,group", CASES)
def test_family_conditions(b, group):
    build = BUILDS[b]
    unit, sites, d = build.groups[group]
    cases = F.load_cases(build, group)
    assert set(cases) == set(F.GROUP_FAMILIES[group])
    total = sum(len(r) for r, _ in cases.values())
    assert 0 < total <= 4096
    z = np.load(build.fixture)
    for fam in cases:       # at most 1 % of a family's pool dropped because the -O2 and the -O3 reference disagree
        died, differed, pool = (int(v) for v in z["%s/%s/dropped" % (group, fam)])
        assert differed * 100 <= pool, (fam, differed, pool)
    n = {}
    if unit == F.A2NLSF:
        n = dict.fromkeys(F.A2NLSF_CLASSES + (F.A2NLSF_BIG,), 0)
        for fam, (recs, out) in cases.items():
            for i in range(len(recs)):
                assert (np.abs(recs[i]) < F.A_Q16_MAX).all()
                r, cs = F.a2nlsf_class(recs[i], out[i], d)
                for c in cs:
                    n[c] += 1
            for i in np.nonzero(z["%s/%s/big_ylo" % (group, fam)])[0]:      # the fixture's mark, checked with the restatement of the whole function
                nl, a_left, retries, big_failed, big = F.a2nlsf_full(recs[i], d)
                assert nl == [int(v) for v in out[i, :d]] and big > 0, (fam, i)
                n[F.A2NLSF_BIG] += 1
        print(group, n)
        for c in F.A2NLSF_CLASSES:
            assert n[c] >= 32, (c, n)
        assert n[F.A2NLSF_BIG] >= 16, n
    elif unit == F.NLSF2A:
        n = dict(ordinary=0, limiter=0, saturated=0, stabilised=0, zero_fallback=0)
        for fam, (recs, out) in cases.items():
            for i in range(len(recs)):
                v = [int(t) for t in recs[i, :d]]
                assert min(v) >= 0 and max(v) <= 32767 and v == sorted(v)
                lim, rounds, sat = F.nlsf2a_limit(F.nlsf2a_a32(v, d))
                declined = int(out[i, 16]) == 1
                assert declined or rounds == 0
                n["ordinary"] += not declined
                n["limiter"] += rounds > 0
                n["saturated"] += sat
                n["stabilised"] += declined and rounds == 0                     # not the limiter: the filter was unstable
                n["zero_fallback"] += declined and not out[i, :d].any() and any(lim)
        print(group, n)
        for c in ("ordinary", "limiter", "stabilised", "zero_fallback"):
            assert n[c] >= 32, (c, n)
    elif unit == F.MSVQ:
        n = dict(tie=0, cut=0, sig0_deact0=0, sig0_deact1=0, sig1_deact0=0, sig1_deact1=0)
        for fam, (recs, out) in cases.items():
            for r in recs:
                assert int(r[51]) in (0, 1) and [int(v) for v in r[32:32 + d]] == F.weights_laroia([int(v) for v in r[:d]], d)
                n["tie"] += F.msvq_stage0_tie(build, r)
                n["cut"] += F.msvq_stage0_cut(build, r)
                n["sig%d_deact%d" % (int(r[48]), int(r[51]))] += 1
        print(group, n)
        assert min(n.values()) >= 16, n
    elif unit == F.BURG:
        sl, nb, D = build.burg_shape(sites[0])
        n = dict(exit=0, rshifts_above_7=0)
        for fam, (recs, out) in cases.items():
            ex = F.burg_exits(build, sites[0], recs)          # (the counting build of the emulation: the outputs do not show the exit)
            for i in range(len(recs)):
                assert not ex[i] or F.burg_exit_order(out[i, 2:], D) > 0           # what the exit leaves in the reference's output
                n["rshifts_above_7"] += F.burg_rshifts(recs[i, :sl * nb]) > 7
            n["exit"] += _count(ex)
        print(group, n)
        assert n["rshifts_above_7"] >= 16, n
        if group == "burg_1" and not build.wb:          # (the module's header: not reached at that site; a family that reaches it belongs here)
            assert n["exit"] == 0, n
        else:
            assert n["exit"] >= 16, n
        assert sum(len(r) for g in ("burg_0", "burg_1", "burg_hb") for r, _ in F.load_cases(build, g).values()) <= 4096
    else:
        n = {"interp%d" % k: 0 for k in range(5)}
        n.update(use_interp0=0, use_interp1=0)
        for fam, (recs, out) in cases.items():
            for i in range(len(recs)):
                n["interp%d" % int(out[i, 16])] += 1
                n["use_interp%d" % int(recs[i, build.X + 16])] += 1
                assert int(recs[i, build.X + 16]) == 1 or int(out[i, 16]) == 4
        # both signs of both energy alignments of the interpolation search, in cases (counters of the emulation's counting build)
        sh = np.concatenate([F.find_lpc_shifts(build, recs) for recs, _ in cases.values()])
        n.update(first_shift_ge0=_count(sh[:, 0] > 0), second_shift_ge0=_count(sh[:, 2] > 0), second_shift_lt0=_count(sh[:, 3] > 0))
        print(group, n, "first_shift_lt0", _count(sh[:, 1] > 0))
        assert min(n.values()) >= 16, n
        # the first shift is never negative: the whole frame's energy contains the second half's, so Burg scales it down at least as far
        assert _count(sh[:, 1] > 0) == 0


@pytest.mark.parametrize("b,group", CASES)
def test_live_reference_equals_fixture(b, group):
    import refcodec as R
    if not (R.have_ref("fix") and R.have_ref("fix_O3")):
        pytest.skip("oracle/_ref is not built")
    build = BUILDS[b]
    for fam, (recs, want) in F.load_cases(build, group).items():
        for kind in ("fix", "fix_O3"):
            got, ok = F.run_ref(build, group, recs, kind, fork=False)
            assert np.array_equal(got, want), (group, fam, kind)


@pytest.mark.parametrize("b", list(BUILDS))
def test_records_and_refusals(b):
    build = BUILDS[b]
    lib = F.load_emu_fn(build.wb)
    assert lib.emu_fn_x_words() == build.X
    for unit in range(5):
        iw, ow = build.words(unit)
        rec, out = np.zeros((1, iw), np.int32), np.zeros((1, ow), np.int32)
        p, q = rec.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
        assert lib.emu_fn(F.fn_id(unit, 0), 1, p, iw, q, ow) == 0
        assert lib.emu_fn(F.fn_id(unit, 0), 1, p, iw + 1, q, ow) == -1 and lib.emu_fn(F.fn_id(unit, 0), 1, p, iw, q, ow - 1) == -1
        assert lib.emu_fn(F.fn_id(unit, 3), 1, p, iw, q, ow) == -1
    assert lib.emu_fn(20, 0, None, 16, None, 32) == -1 and lib.emu_fn(-1, 0, None, 16, None, 32) == -1
    assert lib.emu_fn(F.fn_id(F.NLSF2A, 1), 0, None, 16, None, 17) == -1 and lib.emu_fn(F.fn_id(F.MSVQ, 1), 0, None, 52, None, 32) == -1
    # records that would index a table are not run
    for unit, word, value in ((F.NLSF2A, 3, -1), (F.NLSF2A, 0, 32768), (F.MSVQ, 48, 2), (F.FIND_LPC, build.X + 2, 40000)):
        iw, ow = build.words(unit)
        rec, out = np.zeros((1, iw), np.int32), np.zeros((1, ow), np.int32)
        rec[0, word] = value
        assert lib.emu_fn(F.fn_id(unit, 0), 1, rec.ctypes.data_as(C.c_void_p), iw, out.ctypes.data_as(C.c_void_p), ow) == 0
        assert (out == F.REFUSED).all(), (unit, out)

"""The input families of tests/wave_model.py hold the cases tests/test_gpu_wave_ops.py relies on (wrapping sums, ties inside and
across the 16-lane rows, an idx order that disagrees with the lane order, carries out of the low word inside a row and only across
rows, wrapping prefixes, every hot lane), so that an edit of the generators cannot quietly empty a category.  Also pins the model's
definitions on vectors whose answers are known by hand.  CPU only: the 64-lane forms themselves run on the GPU alone."""
import itertools

import numpy as np

import wave_model as M


def _rows(lanes):
    return np.asarray(lanes) >> 4


def test_model_known_answers():
    v = np.arange(1, 65, dtype=np.int64)[None, :]                     # 1 .. 64
    aux = (63 - M.LANES)[None, :]
    out = M.mode0(v, aux)[0]
    r = {name: out[k] for k, name in enumerate(M.ROWS0)}
    assert (r["wv_sum"] == 2080).all() and (r["wv_max"] == 64).all() and (r["wv_min"] == 1).all()
    assert r["wv_row_sum"].tolist() == [136] * 16 + [392] * 16 + [648] * 16 + [904] * 16
    assert r["wv_col_sum"].tolist() == [4 * j + 100 for j in range(16)] * 4
    assert r["wv_scan_incl"].tolist() == [l * (l + 1) // 2 for l in range(1, 65)]
    assert (r["wv_argmin(idx=lane).idx"] == 0).all() and (r["wv_argmax(idx=lane).idx"] == 63).all()
    assert (r["wv_argmin(idx=aux).idx"] == 63).all() and (r["wv_argmax(idx=aux).idx"] == 0).all()
    # aux[0] = 63: source lane 63, rotation by 63 samples
    assert (r["wv_bcast(v, aux[0] & 63)"] == 64).all() and r["wv_bcast(v, aux & 63)"].tolist() == list(range(64, 0, -1))
    # 64-bit: value of lane l = (63 - l) * 2^32 + (l + 1)
    assert (r["wv_sum64.lo"] == 2080).all() and (r["wv_sum64.hi"] == 2016).all()
    # the LCG, by hand for the first two iterates of seed 63
    x1 = (907633515 + 63 * 196314165) % 2**32
    x2 = (907633515 + x1 * 196314165) % 2**32
    assert int(r["sx_lcg_first"][0]) % 2**32 == x1 and int(r["sx_lcg_first"][1]) % 2**32 == x2
    it = M.lcg_iterates(np.array([63]), 256)[0]
    assert r["sx_lcg_next x3"].tolist() == it[192:].tolist() and r["sx_lcg_next x1"][0] == it[64]
    # lane registers: sample i comes back as sample (i + 63) & 127
    s = [((((j + 1) * 0x9E3779B1) % 2**32) ^ 63) for j in range(128)]
    got = [int(t) % 2**32 for t in r["SX_WRLANE/SX_RDLANE samples 0..63"]] + [int(t) % 2**32 for t in r["SX_WRLANE/SX_RDLANE samples 64..127"]]
    assert got == [s[(i + 63) & 127] for i in range(128)]
    # ties: the smallest idx wins, not the lowest lane
    t = np.zeros((1, 64), np.int64)
    t[0, [5, 40]] = -7
    bv, bi = M.wv_argmin(t, aux)
    assert (bv == -7).all() and (bi == 23).all()                      # lane 40 carries idx 23, lane 5 idx 58
    assert (M.wv_argmin(t, M.LANES[None, :])[1] == 5).all()
    # wraps
    assert (M.wv_sum(np.full((1, 64), M.I32_MAX))[0] == -64).all()
    lo, hi = M.wv_sum64(np.full((1, 64), -1), np.zeros((1, 64)))      # 64 * (2^32 - 1) = 63 * 2^32 + (2^32 - 64)
    assert (lo == -64).all() and (hi == 63).all()


def test_mode1_first_round_is_the_chain():
    f = M.family("A")
    v, aux = f["v"][:64], f["aux"][:64].copy()
    aux[:, 0] = np.arange(64)                                         # every trip count, eight times
    out = M.mode1(v, aux)
    one = (aux[:, 0] & 7) == 0
    assert one.any() and np.array_equal(out[one, :9], out[one, 9:])   # one round: the loop's results are the chain's
    assert not np.array_equal(out[~one, :9], out[~one, 9:])
    # two rounds by hand
    k = int(np.nonzero((aux[:, 0] & 7) == 1)[0][0])
    a, f_, g, hl = (int(out[k, r, 0]) for r in (0, 5, 6, 7))
    x = M.wrap32(v[k:k + 1].astype(np.int64) + a + f_ + g + hl)
    assert np.array_equal(out[k, 9], M.wv_sum(x)[0])


def test_mode2_known_answers():
    # six vectors: one full workgroup and one with two vectors, whose missing half counts as zeros
    v = np.arange(1, 6 * 64 + 1, dtype=np.int64).reshape(6, 64)
    out = M.mode2(v)
    assert out.shape == (6, 3, 64) and out.dtype == np.int32
    r = {name: out[:, k] for k, name in enumerate(M.ROWS2)}
    assert (r["wg_sum"][:4] == 256 * 257 // 2).all() and (r["wg_total"][:4] == 256 * 257 // 2).all()
    assert r["wg_scan_incl"][:4].reshape(-1).tolist() == [l * (l + 1) // 2 for l in range(1, 257)]
    tail = sum(range(257, 385))
    assert (r["wg_sum"][4:] == tail).all() and (r["wg_total"][4:] == tail).all()
    assert r["wg_scan_incl"][4:].reshape(-1).tolist() == [sum(range(257, 257 + l)) for l in range(1, 129)]
    # lane 63 of a vector carries on into lane 0 of the next; the last lane of the workgroup holds the total
    f = M.family("A")["v"][:257]
    out = M.mode2(f)
    assert np.array_equal(out[3::4, 1, 63], out[3::4, 2, 63]) and np.array_equal(out[:, 0], out[:, 2])
    assert np.array_equal(out[1, 1, 0], M.wrap32(np.int64(out[0, 1, 63]) + f[1, 0]))
    assert np.array_equal(out[256, 1], M.wv_scan_incl(f[256:257])[0])              # alone in its workgroup: the wave's scan
    # wraps: 256 lanes of INT32_MAX
    w = M.mode2(np.full((4, 64), M.I32_MAX))
    assert (w[:, 0] == -256).all() and w[:, 1].reshape(-1).tolist() == [int(M.wrap32(np.int64(M.I32_MAX) * l)) for l in range(1, 257)]


def test_workgroup_cases_hold_what_the_gpu_test_relies_on():
    import test_gpu_wave_ops as G
    assert {fam for fam, _ in G.CASES_WG} == {"A", "B", "E"}
    assert sorted(n % 4 for _, n in G.CASES_WG) == [0, 0, 0, 1]
    for fam, n in G.CASES_WG:
        v = M.family(fam)["v"][:n].astype(np.int64)
        assert n <= len(M.family(fam)["tags"])
        if fam == "B":                                                # every hot lane, every extreme
            hot = {int(np.nonzero(x)[0][0]) for x in v if np.count_nonzero(x) == 1}
            assert hot == set(range(64)) and all((v == c).all(axis=1).any() for c in (M.I32_MIN, M.I32_MAX, -1, 0))
        if fam == "E":                                                # wrapping prefixes over the workgroup, one-hot boundary lanes
            pre = np.cumsum(np.concatenate([v, np.zeros((-n % 4, 64), np.int64)]).reshape(-1, 256), axis=1)
            assert ((pre < M.I32_MIN) | (pre > M.I32_MAX)).any(axis=1).sum() >= 32
            assert set(M.BOUNDARY) <= {int(np.nonzero(x)[0][0]) for x in v if np.count_nonzero(x) == 1}


def test_family_a_sums_wrap():
    f = M.family("A")
    s = M.true_sum(f["v"])
    outside = (s < M.I32_MIN) | (s > M.I32_MAX)
    assert 2 * int(outside.sum()) >= len(s)
    assert len(s) % 4 != 0                                            # the last block of four waves is not full


def test_family_b_covers_every_lane_and_extreme():
    f = M.family("B")
    v = f["v"].astype(np.int64)
    for c in (M.I32_MIN, M.I32_MAX, -1, 0):
        assert (v == c).all(axis=1).any(), c
    hot = {val: set() for val in (1, -1, M.I32_MIN, M.I32_MAX)}
    for x in v:
        nz = np.nonzero(x)[0]
        if len(nz) == 1 and int(x[nz[0]]) in hot:
            hot[int(x[nz[0]])].add(int(nz[0]))
    for val, lanes in hot.items():
        assert lanes == set(range(64)), (val, sorted(set(range(64)) - lanes))
    cold = set()
    for x in v:
        other = np.nonzero(x != M.I32_MAX)[0]
        if len(other) == 1:
            cold.add(int(other[0]))
    assert cold == set(range(64))


def test_family_c_ties():
    f = M.family("C")
    v, aux = f["v"].astype(np.int64), f["aux"].astype(np.int64)
    at_min = v == v.min(axis=1, keepdims=True)
    at_max = v == v.max(axis=1, keepdims=True)
    assert ((at_min.sum(axis=1) >= 2) | (at_max.sum(axis=1) >= 2)).all()
    # exactly two lanes at the extreme, in two different rows: every pair of rows, for the minimum and for the maximum
    for at in (at_min, at_max):
        two = np.nonzero(at.sum(axis=1) == 2)[0]
        pairs = {tuple(_rows(np.nonzero(at[k])[0]).tolist()) for k in two}
        for rp in itertools.combinations(range(4), 2):
            assert rp in pairs, rp
        assert any(a == b for a, b in pairs)                          # ... and inside one row
        # every pair of boundary lanes
        lanes = {tuple(np.nonzero(at[k])[0].tolist()) for k in two}
        for pq in itertools.combinations(M.BOUNDARY, 2):
            assert pq in lanes, pq
    # with idx = aux the winner is not always the lowest lane: among two-lane ties, in both orders
    for at, arg in ((at_min, M.wv_argmin), (at_max, M.wv_argmax)):
        two = np.nonzero(at.sum(axis=1) == 2)[0]
        win = arg(v[two], aux[two])[1][:, 0]
        lo_lane = np.array([np.nonzero(at[k])[0][0] for k in two])
        hi_lane = np.array([np.nonzero(at[k])[0][1] for k in two])
        won_hi = win == aux[two, hi_lane]
        won_lo = win == aux[two, lo_lane]
        assert (won_hi ^ won_lo).all()
        assert won_hi.sum() >= 45 and won_lo.sum() >= 45
        # ... also when the two lanes lie in different rows
        cross = _rows(lo_lane) != _rows(hi_lane)
        assert (won_hi & cross).any() and (won_lo & cross).any()
    # many-way ties (values 0 .. 2) where the smallest idx is not in the lowest tied lane
    many = np.nonzero(at_min.sum(axis=1) > 2)[0]
    win = M.wv_argmin(v[many], aux[many])[1][:, 0]
    first = np.array([aux[k, np.nonzero(at_min[k])[0][0]] for k in many])
    assert (win != first).sum() >= 100


def test_family_d_carries():
    f = M.family("D")
    lo = f["v"].astype(np.int64) % 2**32
    per_row = lo.reshape(-1, 4, 16).sum(axis=2)
    total = lo.sum(axis=1)
    for row in range(4):
        assert (per_row[:, row] >= 2**32).any(), row
        # ... exactly 2^32, and with nothing in the other rows
        assert ((per_row[:, row] == 2**32) & (total == 2**32)).any(), row
    only_combined = (per_row < 2**32).all(axis=1) & (total >= 2**32)
    assert only_combined.any()
    # two rows together, each alone below 2^32: every pair of rows
    for ra, rb in itertools.combinations(range(4), 2):
        m = only_combined & (per_row[:, ra] > 0) & (per_row[:, rb] > 0) & (per_row[:, ra] + per_row[:, rb] == total)
        assert m.any(), (ra, rb)
    t = M.true_sum64(f["v"], f["aux"])
    assert any(int(x) < -2**63 or int(x) >= 2**63 for x in t)
    big = f["aux"].astype(np.int64)
    assert (np.abs(big) >= 2**29).any() and ((big == 0) | (big == -1)).any()      # values near +-2^62 and near +-2^31


def test_family_e_scan():
    f = M.family("E")
    v = f["v"].astype(np.int64)
    pre = M.true_scan(v)
    assert ((pre < M.I32_MIN) | (pre > M.I32_MAX)).any(axis=1).sum() >= 100
    ones = np.nonzero((v == 1).all(axis=1))[0]
    assert len(ones) and M.wv_scan_incl(v[ones[:1]])[0].tolist() == list(range(1, 65))
    hot = {int(np.nonzero(x)[0][0]) for x in v if np.count_nonzero(x) == 1}
    assert set(M.BOUNDARY) <= hot


def test_rows_and_shapes():
    assert len(M.ROWS0) == 27 and len(M.ROWS1) == 18 and len(set(M.ROWS0)) == 27 and len(set(M.ROWS1)) == 18 and len(M.ROWS2) == 3
    for name in "ABCDE":
        f = M.family(name)
        n = len(f["tags"])
        assert f["v"].shape == f["aux"].shape == (n, 64) and f["v"].dtype == f["aux"].dtype == np.int32
        assert 64 <= n <= 5000
        assert M.expected(0, name).shape == (n, 27, 64) and M.expected(0, name).dtype == np.int32
    assert M.expected(1, "A").shape == (len(M.family("A")["tags"]), 18, 64)

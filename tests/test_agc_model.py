"""Level control stage (solo_agc, solo_amd/csrc/solo_agc.h) without a GPU: the host form of the kernel source (compiled by this test
from tests/agc_host.cpp) and the independent model of tests/agc_model.py must agree byte for byte in PCM, level_out, gain_q8, count and
the whole state.  No tolerance anywhere, except in test_levels_converge, whose figures come from the model alone."""
import numpy as np
import pytest

import agc_lib as L
import agc_model as M
import vad_lib as VL


@pytest.fixture(scope="module")
def host():
    return L.build_host()


def test_tables_and_lin(host):
    A, B = M.tables()
    assert (A[30], A[60], A[0], B[255], B[0]) == (65536, 2072430, 2072, 73500, 65536)
    assert [host.emu_agc_table_db(i) for i in range(61)] == A and [host.emu_agc_table_frac(r) for r in range(256)] == B
    assert M.lin(0) == 65536 and M.lin(7680) == A[60] and M.lin(-7680) == A[0]
    for d in list(range(-7680, 7681, 97)) + [-7680, -1, 0, 1, 255, 256, 7679, 7680]:
        assert host.emu_agc_lin(d) == M.lin(d), d
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("gen_agc_tables", os.path.join(VL.ROOT, "tools", "gen_agc_tables.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert gen.tables() == (A, B)


def test_lcg_is_the_vad_tests_lcg():
    assert np.array_equal(L.lcg(VL.SEED, 1000), VL.lcg(VL.SEED, 1000)) and np.array_equal(L.noise(5, 300, 87), VL.noise(5, 300, 87))


def test_envelope_closed_form_and_prefix_min(host):
    """the closed form equals the recursion; the six steps of the 64-lane prefix minimum equal a running minimum"""
    r = L.lcg(VL.SEED + 3, 4000).astype(np.int64) >> 8
    at = 0
    for B in (8, 10, 20, 33, 60):
        for rel in (0, 1, 40, 256, 5000, 32768):
            for env in (0, 12345, 32768):
                a = [32768 if v % 3 == 0 else int(v % 32768) for v in r[at:at + B]]
                at = (at + B) % 3900
                assert M.envelope_closed(a, env, rel) == M.envelope(a, env, rel), (B, rel, env)
    for k in range(20):
        v = (L.lcg(VL.SEED + 100 + k, 64).astype(np.int64) >> (8 + k % 16)).astype(np.int32) - 40000 * (k % 3)
        w = v.copy()
        host.emu_agc_prefix_min_steps(w.ctypes.data)
        assert np.array_equal(w, np.minimum.accumulate(v)), k


@pytest.mark.parametrize("shape", L.SHAPES, ids=lambda s: "L%d-n%d-P%d" % s)
def test_host_equals_model_generated(host, shape):
    Ls, n, P = shape
    case = L.generated_case(Ls, n, P)
    L.check_case(L.HostEngine(host, case["n_rows"]), case, shape)


@pytest.mark.parametrize("name", sorted(L.special_cases()))
def test_host_equals_model_special(host, name):
    case = L.special_cases()[name]
    L.check_case(L.HostEngine(host, case["n_rows"]), case, name)


def test_special_cases_show_what_they_are_for():
    """on the model: the cases reach the branch their name says"""
    sc = L.special_cases()

    def outs(name):
        m = M.Agc(sc[name]["n_rows"])
        if "blob" in sc[name]:
            m.set_state_bytes(sc[name]["blob"])
        return m, [m.run(c["pcm"], level=c["level"], sa=c["sa"], rows=c["rows"], **c["prm"]) for c in sc[name]["calls"]]
    for name in ("peak_31", "peak_32", "peak_last", "peak_block0"):
        _, o = outs(name)
        y = o[0]["pcm"][0, 0].astype(int)
        assert np.abs(y).max() == 29204 and o[0]["count"]["limited"] >= 1, name
    _, o = outs("louder_next_packet")
    y = o[0]["pcm"][0].astype(int)
    assert y[0, -1] == 10000 and y[1, 0] == 10000                   # 20000 at 1/2, then 32767 at the step down to a_0
    m, o = outs("slow_release")
    assert [c["count"]["limited"] for c in o] == [1, 1, 1, 0] and int(m.state[0, 4]) == 32768
    _, o = outs("min_sample_max_boost")
    # (|y0| = 1036215 there: the floor in a_b costs up to |y0| / 32768 = 32 of the ceiling)
    assert o[0]["gain"][0, 1] == 7680 and 29204 - 32 <= np.abs(o[0]["pcm"].astype(int)).max() <= 29204
    _, o = outs("falling_ramp")
    g = o[0]["gain"][0]
    assert g[0] > 0 and g[1] < g[0] and g[2] < 0
    _, o = outs("zeros")
    assert not o[0]["pcm"].any() and list(o[0]["level"][0]) == [127, 127] and o[0]["count"]["speech"] == 0 and o[1]["count"]["speech"] == 2
    _, o = outs("level_127")
    assert o[0]["count"]["speech"] == 2 and o[0]["gain"][0, 0] == 128
    _, o = outs("below_sa_on")
    assert o[0]["count"]["speech"] == 2 and o[0]["gain"][0, 1] == o[0]["gain"][0, 0]          # the gain holds in packet 1
    m, o = outs("first_speech")
    assert list(o[0]["gain"][0]) == [0, 128, 256] and o[0]["count"]["speech"] == 2 and int(m.state[0, 1]) == (30 << 8) + 32
    _, o = outs("slew_clamps")
    assert list(o[0]["gain"][0]) == [100, 200, 193]
    _, a = outs("no_level_in")
    _, b = outs("model_level_in")
    assert all(np.array_equal(a[0][k], b[0][k]) for k in ("pcm", "level", "gain"))
    m, o = outs("blob_out_of_range")
    assert np.all(m.state[:, 5:] == 0x5A5A5A5A) and list(m.state[:, 0]) == [7, 1, -1]


def test_packets_in_one_call_equal_calls(host):
    x = L.rows_pcm(VL.SEED, 7, 4, 640)
    sa = L.activities(VL.SEED, 7, 4, 2)
    a, b = L.HostEngine(host, 7), L.HostEngine(host, 7)
    one = a.run(x, None, sa, None, False)
    parts = [b.run(x[:, p:p + 1], None, sa[:, p:p + 1], None, False) for p in range(4)]
    for k in ("pcm", "level", "gain"):
        assert np.array_equal(one[k], np.concatenate([q[k] for q in parts], axis=1)), k
    assert np.array_equal(a.state(), b.state())
    assert one["count"]["speech"] == sum(q["count"]["speech"] for q in parts) and one["count"]["limited"] == sum(q["count"]["limited"] for q in parts)


def test_identity_without_gain_and_limit(host):
    x = np.maximum(L.rows_pcm(VL.SEED, 7, 2, 640), -32767)
    o = L.HostEngine(host, 7).run(x, None, None, None, False, boost=0, cut=0, ceiling=32767)
    assert np.array_equal(o["pcm"], x) and o["count"]["limited"] == 0 and not o["gain"].any()
    assert np.array_equal(M.Agc(7).run(x, boost=0, cut=0, ceiling=32767)["pcm"], x)


def test_lists(host):
    """unlisted rows keep their state; a refused list changes nothing; a list without a count is refused by the host's checks"""
    x = L.rows_pcm(VL.SEED, 3, 2, 320)
    e = L.HostEngine(host, 8)
    sentinel = (np.arange(8 * L.STATE_BYTES, dtype=np.int64) * 37 % 251).astype(np.uint8).reshape(8, L.STATE_BYTES)
    e.set_state(sentinel)
    m = M.Agc(8)
    m.set_state_bytes(sentinel)
    rows = [1, 4, 7]
    got, want = e.run(x, None, None, rows, False), m.run(x, rows=rows)
    assert all(np.array_equal(got[k], want[k]) for k in ("pcm", "level", "gain")) and got["count"] == want["count"]
    st = e.state()
    rest = [0, 2, 3, 5, 6]
    assert np.array_equal(st, m.state_bytes()) and np.array_equal(st[rest], sentinel[rest]) and not np.array_equal(st[rows], sentinel[rows])
    for bad in ([1, 1, 7], [4, 1, 7], [1, 4, 8], [-1, 4, 7]):
        assert e.run(x, None, None, bad, False) is None and e.status == -2 and m.run(x, rows=bad) is None
        assert list(e.raw["count"]) == [-1, 0x5A5A, 0x5A5A, 0x5A5A]
        assert np.all(e.raw["pcm"] == 0x5A5A) and np.all(e.raw["level"] == 0x5A) and np.all(e.raw["gain"] == 0x5A5A)
        assert np.array_equal(e.state(), st)


def test_levels_converge():
    """the speech fixture as 191 packets of 640 samples at three scales 24 dB apart, default parameters, no activity input: the mean
    output level over the second half of each scale's speech packets lies within 2 dB of the target of 23 -dBov, while the input means
    span more than 20 dB.  (The margin covers the >> 3 row, which is still slewing: 18.9 of the 20 dB it wants.)"""
    sp = VL.speech()[:191 * 640].reshape(1, 191, 640)
    scales = [sp, sp >> 3, np.clip(sp << 2, -32768, 32767)]
    means_in, means_out = [], []
    for x in scales:
        x = x.astype(np.int16)
        o = M.Agc(1).run(x)
        lv_in = L.model_levels(x)[0]
        is_speech = np.flatnonzero(lv_in <= M.DEFAULTS["gate"])
        assert len(is_speech) == o["count"]["speech"] >= 100
        half = is_speech[len(is_speech) // 2:]
        means_in.append(float(lv_in[half].mean()))
        means_out.append(float(o["level"][0][half].mean()))
        print("speech packets %d, mean input level %.1f, mean output level %.1f" % (len(is_speech), means_in[-1], means_out[-1]))
    assert all(abs(v - 23) <= 2 for v in means_out), means_out
    assert max(means_in) - min(means_in) > 20, means_in

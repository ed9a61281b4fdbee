"""VAD stage (solo_vad / solo_vad_select, solo_amd/csrc/solo_vad.h) on the GPU, byte for byte against the fixture recorded from the
compiled reference (tests/golden/vad.npz) and the independent model of tests/vad_model.py.  Where a shape goes beyond the fixture the
rows are tiled fixture rows (row i = fixture row i % 6), so the expected data is still the fixture's."""
import ctypes as C

import numpy as np
import pytest

import vad_lib as L
import vad_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(torch, t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def tiled(a, n):
    return a[np.arange(n) % L.ROWS]


def levels(x):
    """model levels of int16 [n, P, Ls] -> uint8 [n, P]"""
    return np.array([[M.level(p) for p in row] for row in x], dtype=np.uint8)


_levels = {}


def fixture_levels():
    if "x" not in _levels:
        _levels["x"] = levels(L.inputs())
    return _levels["x"]


@pytest.mark.parametrize("frame", L.FRAMES)
def test_kernel_equals_fixture(torch_cuda, frame):
    """six rows x 16 packets: one call per packet with the state read after each, then the same rows as one call of 16 packets"""
    import solo_amd
    torch = torch_cuda
    z, x = L.fixture(), dev(torch, L.inputs())
    v = solo_amd.Vad(L.ROWS, frame)
    assert np.array_equal(host(torch, v.get_state()), L.init_state(L.ROWS))
    for p in range(L.PACKETS):
        o = v.run(x[:, p:p + 1].contiguous(), detail=True)
        st = host(torch, v.get_state())
        assert np.array_equal(host(torch, o["sa"])[:, 0], z["sa_%d" % frame][:, p]), (p, "SA")
        assert np.array_equal(host(torch, o["detail"])[:, 0], z["detail_%d" % frame][:, p]), (p, "detail")
        assert np.array_equal(st[:, :L.REF_BYTES], z["state_%d" % frame][:, p]), (p, "state")
        assert not st[:, L.REF_BYTES:].any()
        assert np.array_equal(host(torch, o["level"])[:, 0], fixture_levels()[:, p]), (p, "level")
    last = host(torch, v.get_state())
    v.reset()
    assert np.array_equal(host(torch, v.get_state()), L.init_state(L.ROWS))
    o = v.run(x, detail=True)
    assert np.array_equal(host(torch, o["sa"]), z["sa_%d" % frame]) and np.array_equal(host(torch, o["detail"]), z["detail_%d" % frame])
    assert np.array_equal(host(torch, o["level"]), fixture_levels())
    assert np.array_equal(host(torch, v.get_state()), last)
    # without the optional outputs: the same activities
    v.reset(rows=[1, 4])
    st = host(torch, v.get_state())
    assert np.array_equal(st[[1, 4]], L.init_state(2)) and np.array_equal(st[[0, 2, 3, 5]], last[[0, 2, 3, 5]])
    v.reset()
    o = v.run(x, level=False)
    assert sorted(o) == ["sa"] and np.array_equal(host(torch, o["sa"]), z["sa_%d" % frame])


def test_long_row(torch_cuda):
    """n = 1, 520 packets in one call (1040 frames in sequence, past the counter >= 1000 switch), then the states of the last 32 packets
    from a second run that stops before them"""
    import solo_amd
    torch = torch_cuda
    z, x = L.fixture(), dev(torch, L.long_input()[None])
    v = solo_amd.Vad(1, 320)
    o = v.run(x, level=False)
    assert np.array_equal(host(torch, o["sa"])[0], z["sa_long"])
    assert np.array_equal(host(torch, v.get_state())[0, :L.REF_BYTES], z["state_long"][-1])
    v.reset()
    v.run(x[:, :L.LONG_SQUARE].contiguous(), level=False)
    assert np.array_equal(host(torch, v.get_state())[0, :L.REF_BYTES], z["state_long_square"])
    k = L.LONG_PACKETS - L.LONG_KEPT
    v.run(x[:, L.LONG_SQUARE:k].contiguous(), level=False)
    states = []
    for p in range(k, L.LONG_PACKETS):
        v.run(x[:, p:p + 1].contiguous(), level=False)
        states.append(v.get_state())
    assert np.array_equal(host(torch, torch.cat(states))[:, :L.REF_BYTES], z["state_long"])


@pytest.mark.parametrize("frame,Ls", [(320, 320), (320, 640), (320, 1280), (160, 160), (160, 320)])
@pytest.mark.parametrize("n", [1, 5, 130])
def test_packet_sizes_and_row_counts(torch_cuda, frame, Ls, n):
    import solo_amd
    torch = torch_cuda
    z = L.fixture()
    P = 4 * 640 // Ls
    flat = tiled(L.inputs().reshape(L.ROWS, -1), n)[:, :P * Ls]
    x = flat.reshape(n, P, Ls)
    v = solo_amd.Vad(n, frame)
    o = v.run(dev(torch, x), detail=True)
    nf = P * Ls // frame
    assert np.array_equal(host(torch, o["sa"]).reshape(n, nf), tiled(z["sa_%d" % frame].reshape(L.ROWS, -1), n)[:, :nf])
    assert np.array_equal(host(torch, o["detail"]).reshape(n, nf, 6), tiled(z["detail_%d" % frame].reshape(L.ROWS, -1, 6), n)[:, :nf])
    assert np.array_equal(host(torch, o["level"]), tiled(levels(x[:L.ROWS]), n))
    assert np.array_equal(host(torch, v.get_state())[:, :L.REF_BYTES], tiled(z["state_%d" % frame][:, 3], n))


def test_rows_variant(torch_cuda):
    """64 state rows, 7 listed in compact order; the 57 others hold a sentinel and keep it; bad lists change nothing"""
    import solo_amd
    torch = torch_cuda
    z = L.fixture()
    rows = [3, 4, 17, 31, 32, 62, 63]
    x = dev(torch, tiled(L.inputs(), 7)[:, :3])
    v = solo_amd.Vad(64, 320)
    sentinel = (np.arange(64 * L.STATE_BYTES, dtype=np.int64) * 37 % 251).astype(np.uint8).reshape(64, L.STATE_BYTES)
    v.set_state(dev(torch, sentinel))
    v.reset(rows=rows)
    o = v.run(x, rows=rows, detail=True)
    assert v.count(o["count"]) == dict(rows=7, rooms=0, selected=0, changes=0)
    assert np.array_equal(host(torch, o["sa"]), tiled(z["sa_320"], 7)[:, :3]) and np.array_equal(host(torch, o["detail"]), tiled(z["detail_320"], 7)[:, :3])
    st = host(torch, v.get_state())
    assert np.array_equal(st[rows, :L.REF_BYTES], tiled(z["state_320"], 7)[:, 2]) and not st[rows, L.REF_BYTES:].any()
    rest = np.setdiff1d(np.arange(64), rows)
    assert len(rest) == 57 and np.array_equal(st[rest], sentinel[rest])
    assert np.array_equal(host(torch, v.get_state(rows=[4, 62])), st[[4, 62]])
    # set_state on a list: the listed records, nothing else
    v.set_state(dev(torch, sentinel[[0, 1]]), rows=[17, 40])
    st2 = host(torch, v.get_state())
    assert np.array_equal(st2[[17, 40]], sentinel[[0, 1]]) and np.array_equal(np.delete(st2, [17, 40], axis=0), np.delete(st, [17, 40], axis=0))
    # refused lists (given as device tensors: the host-side check of the Python layer is not what is tested)
    lib = v.lib
    for bad in ([3, 4, 17, 32, 31, 62, 63], [3, 4, 17, 17, 32, 62, 63], [3, 4, 17, 31, 32, 62, 64], [-1, 4, 17, 31, 32, 62, 63]):
        sa = torch.full((7, 3, 2), 0x5A, dtype=torch.uint8, device="cuda")
        det = torch.full((7, 3, 2, 6), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        lev = torch.full((7, 3), 0x5A, dtype=torch.uint8, device="cuda")
        count = torch.full((4,), 0x5A5A, dtype=torch.int32, device="cuda")
        r = lib.solo_vad(v.h, dev(torch, np.array(bad, dtype=np.int32)).data_ptr(), 7, x.data_ptr(), 3, 640, sa.data_ptr(), det.data_ptr(), lev.data_ptr(),
                         count.data_ptr(), v._stream())
        assert r == 0
        assert list(host(torch, count)) == [-1, 0x5A5A, 0x5A5A, 0x5A5A], bad
        assert np.all(host(torch, sa) == 0x5A) and np.all(host(torch, det) == 0x5A5A5A5A) and np.all(host(torch, lev) == 0x5A)
        assert np.array_equal(host(torch, v.get_state()), st2), bad


def test_level_boundaries(torch_cuda):
    """packets whose energy sits on both sides of a threshold: E = c^2 + r ones, c and r chosen per k; zero, one LSB, full scale"""
    import solo_amd
    torch = torch_cuda
    Ls, T_ = 640, M.thresholds()
    packets, want = [], []

    def add(E):
        # E as a sum of squares of int16: greedy big terms, then ones
        x, rest = np.zeros(Ls, dtype=np.int16), E
        for i in range(Ls):
            c = min(int(np.sqrt(rest)), 32767) if rest > 0 else 0
            while c * c > rest:
                c -= 1
            x[i] = c
            rest -= c * c
        assert rest == 0 and int((x.astype(np.int64) ** 2).sum()) == E
        packets.append(x)
        want.append(M.level_of_energy(E, Ls))

    for k in (0, 1, 2, 3, 10, 37, 64, 90, 91, 100, 126, 127):
        e = -((-Ls * T_[k]) >> 20)
        for E in (e - 1, e, e + 1):
            if 0 <= E <= Ls * 32767 ** 2:
                add(E)
    add(0)
    add(1)
    packets.append(np.full(Ls, -32768, dtype=np.int16))
    want.append(0)
    assert len(set(want)) >= 12
    x = np.stack(packets)[:, None, :]
    v = solo_amd.Vad(len(packets), 320)
    o = v.run(dev(torch, x))
    assert list(host(torch, o["level"])[:, 0]) == want


def model_state(m, n_rows):
    st = L.init_state(n_rows).copy()
    st[:, L.REF_BYTES:] = m.state_words().view(np.uint8).reshape(n_rows, 16)
    return st


@pytest.mark.parametrize("prm", L.SELECT_PARAMS, ids=lambda p: "k%d-h%d-s%d" % (p["max_speakers"], p["hang"], p["stick"]))
def test_select_equals_model(torch_cuda, prm):
    """the generated floor of the CPU test (rooms of 1, 2, 3, 65, 200 and an empty one): 8 packets in one call, then 4 one by one"""
    import solo_amd
    torch = torch_cuda
    sa, level, room, gain = L.select_case()
    n, P, _ = sa.shape
    n_rooms = len(L.SELECT_SIZES)
    v, m = solo_amd.Vad(n, 320), M.Select(n)
    for p0, p1 in [(0, 8)] + [(p, p + 1) for p in range(8, P)]:
        want = m.run(sa[:, p0:p1], level[:, p0:p1], room, n_rooms, gain=gain, **prm)
        o = v.select(dev(torch, sa[:, p0:p1]), dev(torch, level[:, p0:p1]), dev(torch, room), n_rooms=n_rooms, gain=dev(torch, gain), **prm)
        inside = room >= 0
        for k in ("sel", "gain_out", "keep"):
            assert np.array_equal(host(torch, o[k])[inside], want[k][inside]), (p0, k)
            assert not host(torch, o[k])[~inside].any(), (p0, k)
        assert np.array_equal(host(torch, o["dominant"]), want["dominant"]), p0
        assert v.count(o["count"]) == want["count"], p0
        assert np.array_equal(host(torch, v.get_state()), model_state(m, n)), p0


def test_select_ties_rows_and_refusals(torch_cuda):
    import solo_amd
    torch = torch_cuda
    sa, level, room = L.tie_case()
    prm = dict(max_speakers=2, on=128, off=64, hang=0, stick=6)
    rows = [1, 2, 3, 5, 8, 9]
    v, m = solo_amd.Vad(10, 160), M.Select(10)
    want = m.run(sa, level, room, 1, rows=rows, **prm)
    o = v.select(dev(torch, sa), dev(torch, level), dev(torch, room), n_rooms=1, rows=rows, **prm)
    got_sel = host(torch, o["sel"])
    for p, exp in enumerate(L.TIE_EXPECTED):
        assert sorted(np.flatnonzero(got_sel[:, p])) == sorted(exp) and host(torch, o["dominant"])[0, p] == exp[0], p
    assert np.array_equal(got_sel, want["sel"]) and v.count(o["count"]) == want["count"]
    assert list(host(torch, o["gain_out"])) == [0, 4096, 0, 0, 4096, 0] and list(host(torch, o["keep"])) == [0, 1, 1, 1, 1, 1]
    st = host(torch, v.get_state())
    assert np.array_equal(st, model_state(m, 10))
    # a bad room id, a bad list: rows = -1, nothing else written, no state moved
    lib = v.lib
    p = solo_amd.solo_vad_select_params_t(2, 128, 64, 0, 6)
    dsa, dlev = dev(torch, sa), dev(torch, level)
    for bad_room, bad_rows in (([0, 0, 0, 0, 0, 1], rows), ([0, 0, -2, 0, 0, 0], rows), (list(room), [1, 2, 3, 5, 8, 10]), (list(room), [1, 2, 3, 3, 8, 9])):
        sel = torch.full((6, 6), 0x5A, dtype=torch.uint8, device="cuda")
        g = torch.full((6,), 0x5A5A, dtype=torch.int16, device="cuda")
        keep = torch.full((6,), 0x5A, dtype=torch.uint8, device="cuda")
        dom = torch.full((1, 6), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        count = torch.full((4,), 0x5A5A, dtype=torch.int32, device="cuda")
        r = lib.solo_vad_select(v.h, dev(torch, np.array(bad_rows, dtype=np.int32)).data_ptr(), 6, dsa.data_ptr(), dlev.data_ptr(), 6, 1,
                                dev(torch, np.array(bad_room, dtype=np.int32)).data_ptr(), 1, C.byref(p), None, sel.data_ptr(), g.data_ptr(), keep.data_ptr(),
                                dom.data_ptr(), count.data_ptr(), v._stream())
        assert r == 0
        assert list(host(torch, count)) == [-1, 0x5A5A, 0x5A5A, 0x5A5A], (bad_room, bad_rows)
        assert np.all(host(torch, sel) == 0x5A) and np.all(host(torch, g) == 0x5A5A) and np.all(host(torch, keep) == 0x5A)
        assert np.all(host(torch, dom) == 0x5A5A5A5A) and np.array_equal(host(torch, v.get_state()), st)


def test_one_tick_end_to_end(torch_cuda):
    """8 rows in 2 rooms, 6 one-packet ticks of the fixture's PCM (packets 2 .. 7): Vad.run, Vad.select with max_speakers 1,
    SoloBatch.mix with the selection's gains -- against tests/mix_model.py evaluated with the model's gains.  Row 0 (speech, silent until
    packet 6), row 1 (stationary noise, which the tracker has learnt by packet 4) and row 3 (zeros) share room 0."""
    import mix_model as MM
    import solo_amd
    torch = torch_cuda
    first, ticks = 2, range(2, 8)
    x = tiled(L.inputs(), 8)
    family = np.arange(8) % L.ROWS                          # 0 = speech, 1 = noise
    room = np.array([0, 0, 1, 0, 1, 1, 1, -1], dtype=np.int32)
    inside = room >= 0
    gain = np.array([4096, 4096, 3000, 4096, 8000, 4096, -5, 4096], dtype=np.int16)
    prm = dict(max_speakers=1, on=128, off=64, hang=2, stick=6)
    b = solo_amd.SoloBatch(8, encoder=False, decoder=True)
    v = solo_amd.Vad(8, 320)
    vm = [M.Vad() for _ in range(8)]
    sm = M.Select(8)
    v.run(dev(torch, x[:, :first]))
    for i in range(8):
        for p in range(first):
            vm[i].packet(x[i, p], 320)
    picked = []
    for p in ticks:
        pcm = dev(torch, x[:, p:p + 1])
        o = v.run(pcm)
        s = v.select(o["sa"], o["level"], dev(torch, room), n_rooms=2, gain=dev(torch, gain), **prm)
        out, count = b.mix(pcm, dev(torch, room), gain=s["gain_out"], max_speakers=64)
        msa = np.stack([vm[i].packet(x[i, p], 320)[0] for i in range(8)])[:, None, :]
        assert np.array_equal(host(torch, o["sa"]), msa), p
        want = sm.run(msa, levels(x[:, p:p + 1]), room, 2, gain=gain, **prm)
        assert np.array_equal(host(torch, s["sel"])[inside], want["sel"][inside]) and np.array_equal(host(torch, s["dominant"]), want["dominant"]), p
        mgain = np.where(inside, want["gain_out"], 0).astype(np.int16)
        assert np.array_equal(host(torch, s["gain_out"]), mgain), p
        ref = MM.model_mix(x[:, p:p + 1], room, 8, gain=mgain, max_speakers=64)
        assert np.array_equal(host(torch, out), ref["out"]), p
        assert b.mix_count(count)["rows"] == 7
        dom = int(want["dominant"][0, 0])
        picked.append(-1 if dom < 0 else int(family[dom]))
        if dom >= 0:
            assert host(torch, s["sel"])[dom, 0] == 1 and host(torch, s["sel"])[room == 0, 0].sum() == 1
    print("room 0, family of the selected row per tick:", picked)
    assert picked[0] == 1                                   # the noise row is what the room hears while nobody speaks and it is not learnt yet
    assert picked[-2:] == [0, 0]                            # ... and once it is learnt and the speech row talks, the speech row

"""Level control stage (solo_agc, solo_amd/csrc/solo_agc.h) on the GPU, byte for byte against the independent model of
tests/agc_model.py: PCM, level_out, gain_q8, count and the whole state after every call, through the C ABI and through solo_amd.Agc,
on the generated cases of tests/agc_lib.py (the same the host build runs in tests/test_agc_model.py)."""
import ctypes as C

import numpy as np
import pytest

import agc_lib as L
import agc_model as M
import vad_lib as VL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch


def dev(torch, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(torch, t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def ptr(t):
    return None if t is None else t.data_ptr()


def params_struct(**prm):
    import solo_amd
    return solo_amd.solo_agc_params_t(*[int(v) for v in M.params_words(**prm)])


class PyEngine:
    """solo_amd.Agc"""

    def __init__(self, torch, n_rows):
        import solo_amd
        self.torch, self.g = torch, solo_amd.Agc(n_rows)

    def state(self):
        return host(self.torch, self.g.get_state())

    def set_state(self, blob):
        self.g.set_state(dev(self.torch, blob))

    def run(self, pcm, level, sa, rows, inplace, **prm):
        t = self.torch
        x = dev(t, pcm)
        y, lo, go, cnt = self.g.run(x, level=dev(t, level), sa=dev(t, sa), rows=rows, out=x if inplace else None, **prm)
        assert not inplace or y.data_ptr() == x.data_ptr()
        if not inplace:
            assert np.array_equal(host(t, x), pcm)          # the input is only read
        return dict(pcm=host(t, y), level=host(t, lo), gain=host(t, go), count=self.g.count(cnt))


class AbiEngine(PyEngine):
    """the C entry point, every buffer the caller's: outputs start from a fill, the rows list is a device tensor as it is"""

    def run(self, pcm, level, sa, rows, inplace, count=True, **prm):
        t, g = self.torch, self.g
        n, P, Ls = pcm.shape
        x, d_level, d_sa = dev(t, pcm), dev(t, level), dev(t, sa)
        y = x if inplace else t.full((n, P, Ls), 0x5A5A, dtype=t.int16, device="cuda")
        lo = t.full((n, P), 0x5A, dtype=t.uint8, device="cuda")
        go = t.full((n, P), 0x5A5A, dtype=t.int16, device="cuda")
        cnt = t.full((4,), 0x5A5A, dtype=t.int32, device="cuda") if count or rows is not None else None
        d_rows = None if rows is None else dev(t, np.array(rows, dtype=np.int32))
        p = params_struct(**prm)
        self.status = g.lib.solo_agc(g.h, ptr(d_rows), n, x.data_ptr(), P, Ls, ptr(d_level), ptr(d_sa), 0 if sa is None else sa.shape[2], C.byref(p),
                                     y.data_ptr(), lo.data_ptr(), go.data_ptr(), ptr(cnt), g._stream())
        self.raw = dict(pcm=host(t, y), level=host(t, lo), gain=host(t, go), count=None if cnt is None else host(t, cnt))
        if self.status or (cnt is not None and self.raw["count"][0] < 0):
            return None
        return dict(self.raw, count=None if cnt is None else dict(zip(g.COUNT, (int(v) for v in self.raw["count"]))))


@pytest.mark.parametrize("engine", [AbiEngine, PyEngine], ids=["abi", "py"])
@pytest.mark.parametrize("shape", L.SHAPES, ids=lambda s: "L%d-n%d-P%d" % s)
def test_kernel_equals_model_generated(torch_cuda, shape, engine):
    Ls, n, P = shape
    case = L.generated_case(Ls, n, P)
    L.check_case(engine(torch_cuda, case["n_rows"]), case, shape)


@pytest.mark.parametrize("name", sorted(L.special_cases()))
def test_kernel_equals_model_special(torch_cuda, name):
    case = L.special_cases()[name]
    L.check_case(AbiEngine(torch_cuda, case["n_rows"]), case, name)


def test_more_rows_than_a_wave_of_blocks(torch_cuda):
    """700 rows (more workgroups than compute units), L = 1920: every lane of the prefix minimum carries a block; without the optional
    outputs; then the resets"""
    torch = torch_cuda
    n, P, Ls = 700, 2, 1920
    x = np.tile(L.rows_pcm(VL.SEED + 5, 14, P, Ls), (50, 1, 1))
    sa = np.tile(L.activities(VL.SEED + 6, 14, P, 6), (50, 1, 1))
    want = M.Agc(14).run(x[:14], sa=sa[:14], release=700, ceiling=9000)
    e = AbiEngine(torch, n)
    got = e.run(x, None, sa, None, False, release=700, ceiling=9000)
    assert np.array_equal(got["pcm"], np.tile(want["pcm"], (50, 1, 1))) and np.array_equal(got["level"], np.tile(want["level"], (50, 1)))
    assert got["count"] == dict(rows=n, speech=50 * want["count"]["speech"], limited=50 * want["count"]["limited"], zero=0)
    assert want["count"]["limited"] > 0 and want["count"]["speech"] > 0
    st = e.state()
    # no level_out, no gain_q8, no count: the same samples and states
    e2 = AbiEngine(torch, n)
    t, g = torch, e2.g
    d_x, d_sa, y = dev(t, x), dev(t, sa), torch.zeros((n, P, Ls), dtype=torch.int16, device="cuda")
    p = params_struct(release=700, ceiling=9000)
    assert g.lib.solo_agc(g.h, None, n, d_x.data_ptr(), P, Ls, None, d_sa.data_ptr(), 6, C.byref(p), y.data_ptr(), None, None, None, g._stream()) == 0
    assert np.array_equal(host(t, y), got["pcm"]) and np.array_equal(e2.state(), st)
    # resets
    init = M.Agc(n).state_bytes()
    g.reset(rows=[699, 3, 64])
    st2 = e2.state()
    assert np.array_equal(st2[[3, 64, 699]], init[:3]) and np.array_equal(np.delete(st2, [3, 64, 699], axis=0), np.delete(st, [3, 64, 699], axis=0))
    g.reset()
    assert np.array_equal(e2.state(), init)
    with pytest.raises(ValueError):
        g.reset(rows=[1, 1])
    with pytest.raises(ValueError):
        g.run(d_x, ceiling=0)


def test_in_place_with_a_list_and_refused_lists(torch_cuda):
    """64 state rows, 7 listed in compact order, in place; the 57 others hold a sentinel and keep it; bad lists change nothing"""
    torch = torch_cuda
    rows = [3, 4, 17, 31, 32, 62, 63]
    x = L.rows_pcm(VL.SEED + 9, 7, 3, 640)
    sentinel = (np.arange(64 * L.STATE_BYTES, dtype=np.int64) * 37 % 251).astype(np.uint8).reshape(64, L.STATE_BYTES)
    e, m = AbiEngine(torch, 64), M.Agc(64)
    e.set_state(sentinel)
    m.set_state_bytes(sentinel)
    e.g.reset(rows=rows)
    m.reset(rows)
    got, want = e.run(x, None, None, rows, True), m.run(x, rows=rows)
    assert all(np.array_equal(got[k], want[k]) for k in ("pcm", "level", "gain")) and got["count"] == want["count"]
    st = e.state()
    rest = np.setdiff1d(np.arange(64), rows)
    assert np.array_equal(st, m.state_bytes()) and len(rest) == 57 and np.array_equal(st[rest], sentinel[rest])
    assert np.array_equal(host(torch, e.g.get_state(rows=[4, 62])), st[[4, 62]])
    # set_state on a list: the listed records, nothing else; an index outside the object moves nothing
    e.g.set_state(dev(torch, sentinel[[0, 1]]), rows=[17, 40])
    m.set_state_bytes(sentinel[[0, 1]], rows=[17, 40])
    st2 = e.state()
    assert np.array_equal(st2[[17, 40]], sentinel[[0, 1]]) and np.array_equal(np.delete(st2, [17, 40], axis=0), np.delete(st, [17, 40], axis=0))
    bad_idx = dev(torch, np.array([5, 64, -1], dtype=np.int32))
    blob = torch.full((3, L.STATE_BYTES), 0x77, dtype=torch.uint8, device="cuda")
    assert e.g.lib.solo_agc_get_state(e.g.h, bad_idx.data_ptr(), 3, blob.data_ptr(), e.g._stream()) == 0
    b = host(torch, blob)
    assert np.array_equal(b[0], st2[5]) and np.all(b[1:] == 0x77)
    # refused lists (device tensors: the host-side check of the Python layer is not what is tested), out of place and in place
    for bad in ([3, 4, 17, 32, 31, 62, 63], [3, 4, 17, 17, 32, 62, 63], [3, 4, 17, 31, 32, 62, 64], [-1, 4, 17, 31, 32, 62, 63]):
        assert e.run(x, None, None, bad, False) is None and e.status == 0
        assert list(e.raw["count"]) == [-1, 0x5A5A, 0x5A5A, 0x5A5A], bad
        assert np.all(e.raw["pcm"] == 0x5A5A) and np.all(e.raw["level"] == 0x5A) and np.all(e.raw["gain"] == 0x5A5A)
        assert e.run(x, None, None, bad, True) is None and np.array_equal(e.raw["pcm"], x)
        assert np.array_equal(e.state(), st2), bad
    # the call after a refused one counts from zero
    got, want = e.run(x, None, None, rows, False), m.run(x, rows=rows)
    assert got["count"]["rows"] == 7 and got["count"] == want["count"] and np.array_equal(got["pcm"], want["pcm"])
    assert np.array_equal(e.state(), m.state_bytes())
    # what the host refuses: -1, nothing enqueued
    g = e.g
    d_x, y = dev(torch, x), torch.zeros((7, 3, 640), dtype=torch.int16, device="cuda")
    d_rows = dev(torch, np.array(rows, dtype=np.int32))
    p = params_struct()
    call = lambda rows=None, n=7, pcm=d_x.data_ptr(), P=3, Ls=640, out=y.data_ptr(), count=None, prm=C.byref(p): \
        g.lib.solo_agc(g.h, rows, n, pcm, P, Ls, None, None, 0, prm, out, None, None, count, g._stream())
    assert call() == 0
    assert call(rows=d_rows.data_ptr()) == -1 and call(n=65) == -1 and call(Ls=648) == -1 and call(pcm=d_x.data_ptr() + 2) == -1
    assert call(out=d_x.data_ptr() + 1280) == -1 and call(prm=None) == -1 and call(pcm=None) == -1 and call(P=0) == -1


def test_graph_replay_equals_calls(torch_cuda):
    """one call captured into a graph and replayed twice = two calls: the state carries from replay to replay"""
    torch = torch_cuda
    n, P, Ls = 5, 2, 640
    x = L.rows_pcm(VL.SEED + 11, n, P, Ls)
    sa = L.activities(VL.SEED + 12, n, P, 2)
    m = M.Agc(n)
    want = [m.run(x, sa=sa, release=300), m.run(x, sa=sa, release=300)]
    e = AbiEngine(torch, n)
    g = e.g
    d_x, d_sa = dev(torch, x), dev(torch, sa)
    y = torch.zeros((n, P, Ls), dtype=torch.int16, device="cuda")
    lo = torch.zeros((n, P), dtype=torch.uint8, device="cuda")
    go = torch.zeros((n, P), dtype=torch.int16, device="cuda")
    cnt = torch.zeros((4,), dtype=torch.int32, device="cuda")
    p = params_struct(release=300)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        r = g.lib.solo_agc(g.h, None, n, d_x.data_ptr(), P, Ls, None, d_sa.data_ptr(), 2, C.byref(p), y.data_ptr(), lo.data_ptr(), go.data_ptr(),
                           cnt.data_ptr(), g._stream())
    assert r == 0
    assert np.array_equal(e.state(), M.Agc(n).state_bytes())                    # captured, not run
    for k in range(2):
        graph.replay()
        assert np.array_equal(host(torch, y), want[k]["pcm"]) and np.array_equal(host(torch, lo), want[k]["level"]), k
        assert np.array_equal(host(torch, go), want[k]["gain"]) and g.count(cnt) == want[k]["count"], k
    assert np.array_equal(e.state(), m.state_bytes())
    assert not np.array_equal(want[0]["pcm"], want[1]["pcm"])


def test_one_tick_end_to_end(torch_cuda):
    """8 rows of the VAD tests' rows in 2 rooms, 10 one-packet ticks: Vad.run, Agc.run on the VAD's level and activity, Vad.select on
    the levelled levels, mix_selected on the levelled rows -- against the same chain with tests/agc_model.py in the stage's place (and
    the models of the other stages in theirs)."""
    import solo_amd
    import vad_model as VM
    from selected_mix_model import model_mix_selected
    torch = torch_cuda
    x = VL.inputs()[np.arange(8) % VL.ROWS].copy()
    x[6] = x[0] >> 3                                        # the same talker as row 0, 18 dB further away
    room = np.array([0, 0, 1, 0, 1, 1, 0, -1], dtype=np.int32)
    prm = dict(max_speakers=2, on=128, off=64, hang=2, stick=6)
    b = solo_amd.SoloBatch(8, encoder=False, decoder=True)
    v, g = solo_amd.Vad(8, 320), solo_amd.Agc(8)
    vm, gm, sm = [VM.Vad() for _ in range(8)], M.Agc(8), VM.Select(8)
    d_room = dev(torch, room)
    gains = []
    for p in range(4, 14):
        pcm = dev(torch, x[:, p:p + 1])
        o = v.run(pcm)
        y, lvl, gain, cnt = g.run(pcm, level=o["level"], sa=o["sa"], up=512)
        s = v.select(o["sa"], lvl, d_room, n_rooms=2, **prm)
        out = b.mix_selected(y, d_room, s["sel"], keep=s["keep"], n_rooms=2)
        msa = np.stack([vm[i].packet(x[i, p], 320)[0] for i in range(8)])[:, None, :]
        mg = gm.run(x[:, p:p + 1], level=L.model_levels(x[:, p:p + 1]), sa=msa, up=512)
        ms = sm.run(msa, mg["level"], room, 2, **prm)
        assert np.array_equal(host(torch, o["sa"]), msa), p
        assert np.array_equal(host(torch, y), mg["pcm"]) and np.array_equal(host(torch, lvl), mg["level"]) and np.array_equal(host(torch, gain), mg["gain"]), p
        assert g.count(cnt) == mg["count"], p
        inside = room >= 0
        assert np.array_equal(host(torch, s["sel"])[inside], ms["sel"][inside]) and np.array_equal(host(torch, s["dominant"]), ms["dominant"]), p
        sel, keep = host(torch, s["sel"]), host(torch, s["keep"])
        want = model_mix_selected(mg["pcm"], room, 2, sel, None, keep)
        c = b.mix_selected_count(out[6])
        assert c == want["count"], (p, c, want["count"])
        ns, nr = c["speakers"], c["shared"]
        for k, i, cut in (("pcm_spk", 0, ns), ("spk_list", 1, ns), ("pcm_room", 3, nr), ("room_list", 4, nr), ("source", 5, 8), ("room_nsel", 7, nr)):
            assert np.array_equal(host(torch, out[i])[:cut], want[k][:cut]), (p, k)
        gains.append([int(q) for q in mg["gain"][:, 0]])
    assert np.array_equal(host(torch, g.get_state()), gm.state_bytes())
    print("gain_q8 per tick, rows 0 and 6:", [(q[0], q[6]) for q in gains])
    assert gains[-1][6] > gains[-1][0] > 0                  # (up = 512: the near talker has arrived) the far talker is raised more
    b.close()

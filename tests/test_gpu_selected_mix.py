"""Shared listener mixes from a given selection on the GPU (solo_mix_selected through the binding and the raw C ABI): everything against
the independent model of tests/selected_mix_model.py on the small families; the identities with solo_mix_shared (its own selection fed
back) and with solo_mix; fewer speakers than the stateless recipe picks; an empty selection; one room of 2048 with 64 speakers spread over
every stride of the gather pass; the refusals; and the tick Vad -> Vad.select -> mix_selected.  All comparisons are exact."""
import ctypes as C

import numpy as np
import pytest

from selected_mix_model import heard, model_mix_selected, selected_case
from shared_mix_model import shared_case

pytestmark = pytest.mark.gpu
FILL = dict(pcm_spk=0x1234, spk_list=-7001, spk_rows=-7002, pcm_room=0x4321, room_list=-7003, source=-7004, room_nsel=0xA5, energy=-77)
OPTIONAL = ("spk_rows", "room_nsel", "energy")
FILL_C = 0x5A5A5A5A
GUARD = 2


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch


def _handle(L, n=4, **kw):
    import solo_amd
    samplerate, framesize_ms = {640: (16000, 40), 1280: (32000, 40), 320: (16000, 20)}[L]
    kw.setdefault("encoder", False)
    h = solo_amd.SoloBatch(n, samplerate=samplerate, framesize_ms=framesize_ms, **kw)
    assert h.packet_samples == L
    return h


def _buffers(torch, n, n_rooms, P, L, guard=GUARD):
    """the outputs of a raw call, pre-filled, with guard rows behind each"""
    dt = dict(pcm_spk=torch.int16, spk_list=torch.int32, spk_rows=torch.int32, pcm_room=torch.int16, room_list=torch.int32, source=torch.int32,
              room_nsel=torch.uint8, energy=torch.int64)
    shapes = dict(pcm_spk=(n + guard, P, L), spk_list=(n + guard,), spk_rows=(n + guard,), pcm_room=(n_rooms + guard, P, L),
                  room_list=(n_rooms + guard,), source=(n + guard,), room_nsel=(n_rooms + guard, P), energy=(n + guard, P))
    b = {k: torch.full(s, FILL[k], dtype=dt[k], device="cuda") for k, s in shapes.items()}
    b["count"] = torch.full((8,), FILL_C, dtype=torch.int32, device="cuda")
    return b


class _Null:
    def data_ptr(self):
        return C.c_void_p(None)


def _raw(h, d_pcm, d_room, n_rooms, d_gain, d_sel, d_keep, d_slots, b, n=None, P=None, drop=()):
    ptr = lambda x: None if x is None else x.data_ptr()
    n = d_pcm.shape[0] if n is None else n
    P = d_pcm.shape[1] if P is None else P
    o = lambda k: None if k in drop else b[k].data_ptr()
    return h.lib.solo_mix_selected(h.h, d_pcm.data_ptr(), n, P, d_room.data_ptr(), n_rooms, ptr(d_gain), ptr(d_sel), ptr(d_keep), ptr(d_slots),
                                   o("pcm_spk"), o("spk_list"), o("spk_rows"), o("pcm_room"), o("room_list"), o("source"), o("room_nsel"),
                                   o("energy"), b["count"].data_ptr(), h._stream())


def _untouched(b, count_from=1):
    return all(bool((b[k] == FILL[k]).all()) for k in FILL) and bool((b["count"][count_from:] == FILL_C).all())


def _compare_raw(torch, h, pcm, room, n_rooms, gain, sel, keep, slots, drop=()):
    """a raw call into pre-filled buffers with guard rows; every array, the fill behind the counts included, against the model"""
    n, P, L = pcm.shape
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    b = _buffers(torch, n, n_rooms, P, L)
    assert _raw(h, up(pcm), up(room), n_rooms, up(gain), up(sel), up(keep), up(slots), b, drop=drop) == 0
    c = h.mix_selected_count(b["count"])
    fill = {k: np.full(tuple(v.shape), FILL[k], v.cpu().numpy().dtype) for k, v in b.items() if k != "count"}
    pad = lambda a, m, v=0: None if a is None else np.concatenate([a, np.full((m - len(a),) + a.shape[1:], v, a.dtype)])
    # (the model sees the guard rows as rows in no room -- selected ones, which do not count -- and as rooms without members)
    want = model_mix_selected(pad(pcm, n + GUARD), pad(room, n + GUARD, -1), n_rooms + GUARD, pad(sel, n + GUARD, 1), pad(gain, n + GUARD),
                              pad(keep, n + GUARD),
                              None if slots is None else np.concatenate([slots, slots[-1] + 1 + np.arange(GUARD, dtype=slots.dtype)]), fill=fill)
    want["source"][want["source"] >= n + GUARD] -= GUARD              # (the call has n rows: the room rows of its table start at n ...
    want["source"][n:] = FILL["source"]                              #  ... and the guards are not even marked -1)
    print("solo_mix_selected %d x %d x %d: count %s" % (n, P, L, c))
    assert c == want["count"], (c, want["count"])
    for k in FILL:
        got = b[k].cpu().numpy()
        if k in drop:
            assert (got == FILL[k]).all(), k
        else:
            bad = np.argwhere(got != want[k])
            assert len(bad) == 0, (k, bad[:6].tolist())
    return want


@pytest.mark.parametrize("L,P", [(320, 3), (640, 1), (640, 3), (1280, 1), (1280, 3)])
def test_gpu_mix_selected_against_model(torch_cuda, L, P):
    """the small family with everything the interface names, n <= 256: once with everything optional given, once with all of it NULL"""
    torch = torch_cuda
    pcm, room, gain, n_rooms, sel, keep, slots, marks = selected_case(900 + L + P, P, L)
    assert len(room) <= 256
    h = _handle(L)
    want = _compare_raw(torch, h, pcm, room, n_rooms, gain, sel, keep, slots)
    c = want["count"]
    assert c["clipped"] > 0 and c["silent"] > 0 and 0 < c["shared"] < c["rooms"] and 0 < c["speakers"] < c["rows"] and c["selected"] >= 64
    _compare_raw(torch, h, pcm, room, n_rooms, None, sel, None, None, drop=OPTIONAL)
    # through the binding
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out = h.mix_selected(up(pcm), up(room), up(sel), gain=up(gain), keep=up(keep), slots=up(slots), n_rooms=n_rooms)
    assert h.mix_selected_count(out[6]) == c and tuple(out[7].shape) == (n_rooms, P)
    ns, nr = c["speakers"], c["shared"]
    for k, i, m in (("pcm_spk", 0, ns), ("spk_list", 1, ns), ("spk_rows", 2, ns), ("pcm_room", 3, nr), ("room_list", 4, nr), ("room_nsel", 7, nr)):
        assert np.array_equal(out[i].cpu().numpy()[:m], want[k][:m]), k
    assert np.array_equal(out[5].cpu().numpy(), want["source"][:len(room)])
    h.close()


@pytest.mark.parametrize("K", [1, 2, 3])
def test_gpu_selection_of_mix_shared_gives_mix_shared(torch_cuda, K):
    """sel := d_mixed of a solo_mix_shared call on the same arguments: every common output and the five common counts are equal"""
    torch = torch_cuda
    P, L = 3, 640
    pcm, room, gain, n_rooms, keep, slots, _ = shared_case(1000 + K, P, L, K)
    n = len(room)
    h = _handle(L)
    d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (pcm, room, gain, keep, slots)]
    mixed = torch.zeros((n, P), dtype=torch.uint8, device="cuda")            # (rows in no room stay 0)
    energy = torch.zeros((n, P), dtype=torch.int64, device="cuda")
    a = h.mix_shared(d[0], d[1], gain=d[2], max_speakers=K, keep=d[3], slots=d[4], n_rooms=n_rooms, mixed=mixed, energy=energy)
    energy2 = torch.zeros((n, P), dtype=torch.int64, device="cuda")
    b = h.mix_selected(d[0], d[1], mixed, gain=d[2], keep=d[3], slots=d[4], n_rooms=n_rooms, energy=energy2)
    ca, cb = h.mix_shared_count(a[6]), h.mix_selected_count(b[6])
    assert {k: cb[k] for k in ca} == ca and ca["speakers"] > 0 and ca["shared"] > 0 and cb["selected"] == int(mixed.sum())
    for i, m in ((0, ca["speakers"]), (1, ca["speakers"]), (2, ca["speakers"]), (3, ca["shared"]), (4, ca["shared"]), (5, n)):
        assert torch.equal(a[i][:m], b[i][:m]), i
    assert torch.equal(energy, energy2)
    h.close()


@pytest.mark.parametrize("L", [320, 640, 1280])
def test_gpu_everybody_hears_what_solo_mix_gives(torch_cuda, L):
    """at P = 1 every row hears through `source` what solo_mix gives it with the gains sel ? gain : 0 and max_speakers = 64"""
    torch = torch_cuda
    pcm, room, gain, n_rooms, sel, keep, slots, _ = selected_case(1100 + L, 1, L)
    n = len(room)
    h = _handle(L)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_pcm, d_room = up(pcm), up(room)
    out = h.mix_selected(d_pcm, d_room, up(sel), gain=up(gain), keep=up(keep), n_rooms=n_rooms)
    ref, _ = h.mix(d_pcm, d_room, gain=up(np.where(sel[:, 0] != 0, gain, 0).astype(np.int16)), max_speakers=64)
    got = dict(pcm_spk=out[0].cpu().numpy(), pcm_room=out[3].cpu().numpy(), source=out[5].cpu().numpy())
    assert np.array_equal(heard(got, n)[room >= 0], ref.cpu().numpy()[room >= 0])
    h.close()


def test_gpu_fewer_speakers_than_the_stateless_recipe(torch_cuda):
    """rooms of 8, one selected member each, no keep: one speaker and one room row per room, where solo_mix_shared under the masked gains
    and max_speakers = 3 makes three speakers per room -- and every row hears the same samples in both"""
    torch = torch_cuda
    rng = np.random.default_rng(5)
    rooms, P, L = 16, 2, 640
    n = rooms * 8
    room = np.repeat(np.arange(rooms), 8).astype(np.int32)[rng.permutation(n)]
    pcm = (rng.integers(-32768, 32768, (n, P, L)) >> rng.integers(0, 8, (n, 1, 1))).astype(np.int16)
    gain = rng.integers(1000, 8192, n).astype(np.int16)
    sel = np.zeros((n, P), np.uint8)
    for r in range(rooms):
        sel[np.flatnonzero(room == r)[r % 8]] = 1
    h = _handle(L)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_pcm, d_room = up(pcm), up(room)
    a = h.mix_selected(d_pcm, d_room, up(sel), gain=up(gain), n_rooms=rooms)
    ca = h.mix_selected_count(a[6])
    assert ca["speakers"] == rooms and ca["shared"] == rooms and ca["selected"] == rooms * P and ca["silent"] == 0
    assert bool((a[7] == 1).all())
    b = h.mix_shared(d_pcm, d_room, gain=up(np.where(sel[:, -1] != 0, gain, 0).astype(np.int16)), max_speakers=3, n_rooms=rooms)
    cb = h.mix_shared_count(b[6])
    assert cb["speakers"] == 3 * rooms and cb["shared"] == rooms
    table = lambda o: dict(pcm_spk=o[0].cpu().numpy(), pcm_room=o[3].cpu().numpy(), source=o[5].cpu().numpy())
    assert np.array_equal(heard(table(a), n), heard(table(b), n))
    want = model_mix_selected(pcm, room, rooms, sel, gain)
    assert np.array_equal(heard(table(a), n), heard(want, n)) and ca == want["count"]
    h.close()


def test_gpu_empty_selection(torch_cuda):
    """nobody speaks: zero room rows, room_nsel 0, silent = shared x P, and the speakers d_keep keeps hear zeros"""
    torch = torch_cuda
    rng = np.random.default_rng(6)
    rooms, P, L = 9, 3, 640
    n = rooms * 5 + 3
    room = np.concatenate([np.repeat(np.arange(rooms), 5), [-1, -1, -1]]).astype(np.int32)[rng.permutation(n)]
    pcm = rng.integers(-32768, 32768, (n, P, L)).astype(np.int16)
    sel = np.zeros((n, P), np.uint8)
    sel[room < 0] = 1                                                          # (rows in no room do not count)
    keep = np.zeros(n, np.uint8)
    keep[np.flatnonzero(room == 2)] = 1                                        # a room of kept speakers only: not shared
    keep[np.flatnonzero(room == 4)[:2]] = 1
    h = _handle(L)
    want = _compare_raw(torch, h, pcm, room, rooms, None, sel, keep, None)
    c = want["count"]
    assert c["speakers"] == 7 and c["shared"] == rooms - 1 and c["selected"] == 0 and c["silent"] == c["shared"] * P and c["clipped"] == 0
    assert not want["pcm_room"][:c["shared"]].any() and not want["room_nsel"][:c["shared"]].any() and not want["pcm_spk"][:7].any()
    h.close()


def _large_room():
    """one room of 2048, 64 selected: one in every run of 64 rows (what a stride of the gather pass covers when the member list is in
    row order, which the scatter follows closely), a second one in 27 of them, five more in one run; two of the selected are identical
    full-scale rows and the others are quiet, so S saturates; two kept rows that are not selected"""
    rng = np.random.default_rng(78)
    n, P, L = 2048, 1, 640
    picks = sorted([64 * s + 7 for s in range(32)] + [64 * s + 40 for s in range(27)] + [64 * 5 + 10 + j for j in range(5)])
    assert len(set(picks)) == 64
    pcm = (rng.integers(-32768, 32768, (n, P, L), dtype=np.int16) >> rng.integers(0, 10, (n, P, 1))).astype(np.int16)
    pcm[picks] >>= 7
    pcm[[picks[3], picks[50]]] = 32767
    gain = rng.integers(-100, 8192, n).astype(np.int16)
    gain[picks] = 4096
    sel = np.zeros((n, P), np.uint8)
    sel[picks] = 1
    keep = np.zeros(n, np.uint8)
    keep[[5, 2047]] = 1
    return pcm, np.zeros(n, np.int32), gain, sel, keep, picks


def test_gpu_one_large_room(torch_cuda):
    torch = torch_cuda
    pcm, room, gain, sel, keep, picks = _large_room()
    n = len(room)
    h = _handle(640)
    want = _compare_raw(torch, h, pcm, room, 1, gain, sel, keep, None)
    c = want["count"]
    assert c == dict(rows=n, rooms=1, speakers=66, shared=1, clipped=c["clipped"], selected=64, silent=0) and c["clipped"] >= 640
    assert want["spk_rows"][:66].tolist() == sorted(picks + [5, 2047]) and want["room_nsel"][0, 0] == 64
    h.close()


def test_gpu_mix_selected_refusals(torch_cuda):
    """the host refuses with -1 and enqueues nothing; a device refusal writes rows = -1 and nothing else"""
    torch = torch_cuda
    P, L = 2, 640
    pcm, room, gain, n_rooms, sel, keep, slots, _ = selected_case(15, P, L, big=12)
    n = len(room)
    h = _handle(L)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_pcm, d_room, d_sel, d_slots = up(pcm), up(room), up(sel), up(slots)
    b = _buffers(torch, n, n_rooms, P, L)
    call = lambda n_rooms=n_rooms, bufs=b, pin=d_pcm, sel=d_sel, **kw: _raw(h, pin, d_room, n_rooms, None, sel, None, d_slots, bufs, **kw)
    assert call(n_rooms=0) == -1 and call(n_rooms=n + 1) == -1 and call(n=0) == -1 and call(P=0) == -1
    assert call(n=2, P=2 ** 30, n_rooms=1) == -1
    assert call(sel=None) == -1                                                                  # the selection is required
    assert call(bufs=dict(b, pcm_spk=b["pcm_spk"][0, 0, 4:])) == -1                               # not 16-byte aligned
    assert call(bufs=dict(b, pcm_room=d_pcm)) == -1 and call(bufs=dict(b, pcm_spk=d_pcm[n - 1:])) == -1          # overlap with the input
    assert call(bufs=dict(b, pcm_room=b["pcm_spk"][n - 1:])) == -1                                # ... and of the outputs
    for k in ("pcm_spk", "spk_list", "pcm_room", "room_list", "source", "count"):
        assert call(bufs=dict(b, **{k: _Null()})) == -1, k
    torch.cuda.synchronize()
    assert _untouched(b, 0)
    for what in ("room_low", "room_high", "slots_negative", "slots_equal"):
        r2, s2 = room.copy(), slots.copy()
        if what == "room_low":
            r2[3] = -2
        elif what == "room_high":
            r2[n - 1] = n_rooms
        elif what == "slots_negative":
            s2[0] = -1
        else:
            s2[n - 1] = s2[n - 2]
        assert _raw(h, d_pcm, up(r2), n_rooms, None, d_sel, None, up(s2), b) == 0
        torch.cuda.synchronize()
        assert int(b["count"][0]) == -1 and _untouched(b), what
        assert h.mix_selected_count(b["count"])["rows"] == -1
        b["count"][0] = FILL_C
    # the handle mixes on afterwards
    assert call() == 0
    assert h.mix_selected_count(b["count"])["rows"] == int((room >= 0).sum())
    # the room of 2048 with a 65th member selected
    pcm, room, gain, sel, keep, picks = _large_room()
    sel[1001] = 1
    assert not keep[1001] and 1001 not in picks
    b = _buffers(torch, 2048, 1, 1, L)
    assert _raw(h, up(pcm), up(room), 1, up(gain), up(sel), up(keep), None, b) == 0
    torch.cuda.synchronize()
    assert int(b["count"][0]) == -1 and _untouched(b)
    assert model_mix_selected(pcm, room, 1, sel, gain, keep)["count"]["rows"] == -1
    h.close()


def test_gpu_tick_vad_select_mix_selected(torch_cuda):
    """Vad on synthetic rows -> Vad.select -> mix_selected, four packets in one call and as four calls of one packet: the selections
    agree, every one-packet call gives what the model makes of the selection and the candidates it was handed, and `selected` is the
    count solo_vad_select reports"""
    import solo_amd
    from solo_amd.synth import synth_batch
    torch = torch_cuda
    rng = np.random.default_rng(9)
    n, T_, L, n_rooms = 40, 4, 640, 6
    room = np.concatenate([np.repeat(np.arange(n_rooms), (1, 2, 5, 8, 8, 14)), [-1, -1]]).astype(np.int32)[rng.permutation(n)]
    talk = rng.random((n, T_)) < 0.4
    talk[np.flatnonzero(room == 3)] = False                                    # a room in which nobody ever talks
    x = synth_batch(300, n, T_)
    x = np.where(talk[:, :, None], x, 0).astype(np.int16)                      # those who do not talk send digital silence
    h = _handle(L)
    d_room = torch.from_numpy(room).cuda()
    d_x = torch.from_numpy(x).cuda()
    # four packets in one call
    vad = solo_amd.Vad(n, 320)
    v = vad.run(d_x)
    s = vad.select(v["sa"], v["level"], d_room, n_rooms=n_rooms, max_speakers=3)
    out = h.mix_selected(d_x, d_room, s["sel"], keep=s["keep"], n_rooms=n_rooms)
    vc, c = vad.count(s["count"]), h.mix_selected_count(out[6])
    sel_all, keep_all = s["sel"].cpu().numpy(), s["keep"].cpu().numpy()
    want = model_mix_selected(x, room, n_rooms, sel_all, None, keep_all)
    print("tick, one call: vad %s, mix %s" % (vc, c))
    assert c == want["count"] and c["selected"] == vc["selected"] > 0 and c["silent"] >= T_ and c["rows"] == vc["rows"]
    ns, nr = c["speakers"], c["shared"]
    for k, i, m in (("pcm_spk", 0, ns), ("spk_list", 1, ns), ("pcm_room", 3, nr), ("room_list", 4, nr), ("source", 5, n), ("room_nsel", 7, nr)):
        assert np.array_equal(out[i].cpu().numpy()[:m], want[k][:m]), k
    # ... and as four calls of one packet
    vad1 = solo_amd.Vad(n, 320)
    selected = 0
    for t in range(T_):
        d_xt = d_x[:, t:t + 1].contiguous()
        v = vad1.run(d_xt)
        s = vad1.select(v["sa"], v["level"], d_room, n_rooms=n_rooms, max_speakers=3)
        out = h.mix_selected(d_xt, d_room, s["sel"], keep=s["keep"], n_rooms=n_rooms)
        vc, c = vad1.count(s["count"]), h.mix_selected_count(out[6])
        sel_t, keep_t = s["sel"].cpu().numpy(), s["keep"].cpu().numpy()
        assert np.array_equal(sel_t[:, 0], sel_all[:, t]), t                   # P packets in one call = P calls of one packet
        want = model_mix_selected(x[:, t:t + 1], room, n_rooms, sel_t, None, keep_t)
        assert c == want["count"] and c["selected"] == vc["selected"], (t, c, want["count"], vc)
        ns, nr = c["speakers"], c["shared"]
        for k, i, m in (("pcm_spk", 0, ns), ("spk_list", 1, ns), ("pcm_room", 3, nr), ("room_list", 4, nr), ("source", 5, n), ("room_nsel", 7, nr)):
            assert np.array_equal(out[i].cpu().numpy()[:m], want[k][:m]), (t, k)
        selected += c["selected"]
    assert selected == int((sel_all[room >= 0] != 0).sum()) > 0
    assert np.array_equal(keep_t, keep_all)
    h.close()

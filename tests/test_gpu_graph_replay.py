"""Graph capture and replay of the calls a bridge tick is made of (include/solo_mi355x.h, "Graph capture").

Every test captures with torch.cuda.graph (default error mode) on buffers allocated once, after one eager call of the same geometry
(the handle's one-time set-up and its scratch), calls the library through the C ABI, rewrites the inputs in place between replays and
compares bit for bit:
  1  every stage alone: each replay against the same call made eagerly on a twin object, and against the Python model of the stage;
  2  the codec calls: against the reference's bitstreams and its decoder's PCM (tests/golden/synth8x25.npz, enc_stages_wb.npz);
  3  eager calls and replays interleaved on one handle, following the fixture's 25 packets;
  4  the bridge tick in one graph against twin handles running the same ticks eagerly.
CAPTURED names, for every entry point the interface calls capturable, the test that captures it (tests/test_graph_claims.py holds the
header to it)."""
import ctypes as C

import numpy as np
import pytest

import agc_model as AM
import graph_replay_lib as G
import playout_lib as PL
import playout_model as PM
import resample_lib as RL
import resample_model as RM
import solo_testlib as T
import vad_lib as VL
import vad_model as VM
from mix_model import model_mix
from recv_report_model import RingModel
from selected_mix_model import model_mix_selected
from send_pack_model import model_pack
from shared_mix_model import fanout_case, model_fanout, model_mix_shared
from timescale_model import geometry, model_timescale, timescale_rows

pytestmark = pytest.mark.gpu

# entry point -> the test below that captures it
CAPTURED = {
    "solo_resample": "test_resample", "solo_resample_rows": "test_resample_rows",
    "solo_vad": "test_vad", "solo_vad_select": "test_vad_select",
    "solo_timescale": "test_timescale",
    "solo_mix": "test_mix", "solo_mix_shared": "test_mix_shared", "solo_mix_selected": "test_mix_selected",
    "solo_send_pack": "test_send_pack_device_sequence_base", "solo_send_pack_streams": "test_send_pack_streams",
    "solo_send_fanout": "test_send_fanout",
    "solo_recv_report": "test_recv_report_with_a_play_list", "solo_recv_insert": "test_recv_insert_fixed_capacity",
    "solo_recv_decode": "test_recv_decode", "solo_recv_decode_streams": "test_recv_decode_streams",
    "solo_playout_plan": "test_playout_plan", "solo_playout_render": "test_playout_render",
    "solo_agc": "test_bridge_tick_in_one_graph",             # (alone: tests/test_gpu_agc.py::test_graph_replay_equals_calls)
    "solo_batch_encode": "test_encode", "solo_batch_decode": "test_decode", "solo_batch_decode_split": "test_decode_split",
    "solo_batch_encode_streams": "test_encode_streams", "solo_batch_decode_streams": "test_decode_streams",
    "solo_batch_wait_encode": "test_encode_async_join",
}
# declared under a comment that speaks of capture, but not captured: the lifecycle of the objects (the header says that everything a
# handle or an object sets up once comes before a capture) and the calls that read on the host
NOT_CAPTURED = {
    "solo_recv_track": "allocates the counters on first use",
    "solo_playout_tick": "reads the plan's count on the host",
    "solo_playout_gather": "a plain row copy between plan and render; the tick that needs it is not capturable",
    "solo_resample_out_samples": "host arithmetic",
    "solo_recv_create": "allocates the ring and synchronises", "solo_recv_stats": "copies to the host",
    "solo_batch_set_async_join": "a host switch, read when a call is issued",
}
for _p in ("resample", "vad", "playout", "agc"):
    for _f in ("create", "destroy", "reset", "reset_rows") + (("get_state", "set_state") if _p != "resample" else ()):
        NOT_CAPTURED["solo_%s_%s" % (_p, _f)] = "lifecycle of the object: before a capture"

N, L, SLOT = 8, 640, 512


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


def ptr(t):
    return None if t is None else t.data_ptr()


def count_of(struct, a):
    c = struct.from_buffer_copy(np.ascontiguousarray(a).tobytes())
    return {k: int(getattr(c, k)) for k, _ in struct._fields_}


def beyond(a, k, fill):
    """entries k.. still hold the fill"""
    return bool((np.asarray(a)[k:] == fill).all())


def handle(**kw):
    import solo_amd
    kw.setdefault("encoder", False)
    return solo_amd.SoloBatch(N, slot_bytes=SLOT, **kw)


# ==== 1. every stage alone =====================================================================================================================
def _resample(torch, pair, lists):
    """5 rows, one packet of 40 ms per call; lists: None, or the device list of each call (3 of the 5 rows, same length, other contents)"""
    import solo_amd
    fs_in, fs_out = pair
    x, n = RL.inputs(fs_in)[:5], 5 if lists is None else 3
    Li = x.shape[2]
    Lo = Li * fs_out // fs_in
    assert Li == {48000: 1920, 16000: 640}[fs_in]
    made = []

    def make():
        rs = solo_amd.Resampler(5, fs_in, fs_out)
        ins = dict(x=G.zeros(torch, (n, 1, Li), torch.int16))
        outs = dict(y=G.zeros(torch, (n, 1, Lo), torch.int16))
        if lists is None:
            call = lambda: rs.lib.solo_resample(rs.h, ins["x"].data_ptr(), 1, Li, outs["y"].data_ptr(), rs._stream())
        else:
            ins["rows"] = G.zeros(torch, (n,), torch.int32)
            outs["count"] = G.zeros(torch, (2,), torch.int32)
            call = lambda: rs.lib.solo_resample_rows(rs.h, ins["rows"].data_ptr(), n, ins["x"].data_ptr(), 1, Li, outs["y"].data_ptr(),
                                                     outs["count"].data_ptr(), rs._stream())
        made.append(rs)
        return G.Stage(torch, ins, outs, call, keep=rs)

    rows_of = lambda k: list(range(5)) if lists is None else lists[k]
    feeds = [dict(x=x[rows_of(k), k:k + 1]) for k in range(4)]
    if lists is not None:
        for k in range(4):
            feeds[k]["rows"] = np.array(lists[k], np.int32)
    state = {"st": np.zeros((5, RL.STATE_BYTES), np.uint8)}

    def model(k, feed, got):
        r = rows_of(k)
        want, st = RM.run_rows(fs_in, fs_out, feed["x"], state["st"][r])
        state["st"][r] = st
        assert np.array_equal(got["y"], want), k
        if lists is not None:
            assert got["count"].tolist() == [n, n]

    G.replay_against_twin(torch, make, feeds, model=model)
    # the state the replays left: a packet of zeros through all five rows, eagerly, on both
    tail = [host(torch, rs.run(G.zeros(torch, (5, 1, Li), torch.int16))) for rs in made]
    want, _ = RM.run_rows(fs_in, fs_out, np.zeros((5, 1, Li), np.int16), state["st"])
    assert np.array_equal(tail[0], tail[1]) and np.array_equal(tail[0], want) and tail[0].any()


@pytest.mark.parametrize("pair", ((48000, 16000), (16000, 48000)), ids=lambda p: "%d-%d" % (p[0] // 1000, p[1] // 1000))
def test_resample(torch_cuda, pair):
    """packets of 1920 and of 640 samples; the filter memory carries from replay to replay"""
    _resample(torch_cuda, pair, None)


def test_resample_rows(torch_cuda):
    """the device list changes between replays and keeps its length: every row continues from its own memory"""
    _resample(torch_cuda, (48000, 16000), ([0, 2, 3], [1, 2, 4], [0, 1, 4], [2, 3, 4]))


def _vad_pcm():
    return VL.inputs()[np.arange(N) % VL.ROWS][:, 4:8]                    # [8, 4, 640]: onset and speech of the fixture's rows


def test_vad(torch_cuda):
    import solo_amd
    torch = torch_cuda
    x = _vad_pcm()

    def make():
        v = solo_amd.Vad(N, 320)
        ins = dict(x=G.zeros(torch, (N, 1, L), torch.int16))
        outs = dict(sa=G.zeros(torch, (N, 1, 2), torch.uint8), detail=G.zeros(torch, (N, 1, 2, 6), torch.int32), level=G.zeros(torch, (N, 1), torch.uint8),
                    count=G.zeros(torch, (4,), torch.int32))
        call = lambda: v.lib.solo_vad(v.h, None, N, ins["x"].data_ptr(), 1, L, outs["sa"].data_ptr(), outs["detail"].data_ptr(), outs["level"].data_ptr(),
                                      outs["count"].data_ptr(), v._stream())
        return G.Stage(torch, ins, outs, call, state=lambda: host(torch, v.get_state()), keep=v)

    vm = [VM.Vad() for _ in range(N)]

    def model(k, feed, got):
        for i in range(N):
            sa, detail = vm[i].packet(feed["x"][i, 0], 320)
            assert np.array_equal(got["sa"][i, 0], sa) and np.array_equal(got["detail"][i, 0], detail), (k, i)
            assert got["level"][i, 0] == VM.level(feed["x"][i, 0]), (k, i)
        assert got["count"].tolist() == [N, 0, 0, 0]

    _, cap, _ = G.replay_against_twin(torch, make, [dict(x=x[:, k:k + 1]) for k in range(4)], model=model, stateful=True)
    assert np.array_equal(cap.state()[:, :VL.REF_BYTES], np.stack([m.state_bytes() for m in vm]))


def test_vad_select(torch_cuda):
    """two packets a call; the room ids are a device buffer and move between replays like the activities and the levels"""
    import solo_amd
    torch = torch_cuda
    P, F = 2, 2
    sa, level = VL.select_streams(VL.SEED + 40, N, 4 * P, F)
    rooms = [np.array(r, np.int32) for r in ([0, 0, 1, 0, 1, 1, 0, -1], [0, 1, 1, 0, 1, -1, 0, 0], [1, 0, 1, 0, 1, 1, 0, 0], [0, 0, 1, 1, 1, 1, -1, 0])]
    prm = dict(max_speakers=2, on=128, off=64, hang=1, stick=6)

    def make():
        v = solo_amd.Vad(N, 320)
        ins = dict(sa=G.zeros(torch, (N, P, F), torch.uint8), level=G.zeros(torch, (N, P), torch.uint8), room=G.zeros(torch, (N,), torch.int32))
        outs = dict(sel=G.zeros(torch, (N, P), torch.uint8), gain_out=G.zeros(torch, (N,), torch.int16), keep=G.zeros(torch, (N,), torch.uint8),
                    dominant=G.zeros(torch, (2, P), torch.int32), count=G.zeros(torch, (4,), torch.int32))
        p = solo_amd.solo_vad_select_params_t(prm["max_speakers"], prm["on"], prm["off"], prm["hang"], prm["stick"])
        call = lambda: v.lib.solo_vad_select(v.h, None, N, ins["sa"].data_ptr(), ins["level"].data_ptr(), P, F, ins["room"].data_ptr(), 2, C.byref(p), None,
                                             outs["sel"].data_ptr(), outs["gain_out"].data_ptr(), outs["keep"].data_ptr(), outs["dominant"].data_ptr(),
                                             outs["count"].data_ptr(), v._stream())
        return G.Stage(torch, ins, outs, call, state=lambda: host(torch, v.get_state()), keep=v)

    sm = VM.Select(N)

    def model(k, feed, got):
        want = sm.run(feed["sa"], feed["level"], feed["room"], 2, **prm)
        for key in ("sel", "gain_out", "keep", "dominant"):
            assert np.array_equal(got[key], want[key]), (k, key)
        assert count_of(solo_amd.solo_vad_count_t, got["count"]) == want["count"], k

    feeds = [dict(sa=sa[:, k * P:(k + 1) * P], level=level[:, k * P:(k + 1) * P], room=rooms[k]) for k in range(4)]
    _, cap, _ = G.replay_against_twin(torch, make, feeds, model=model, stateful=True)
    assert np.array_equal(np.ascontiguousarray(cap.state()[:, VL.REF_BYTES:]).view(np.int32), sm.state_words())


@pytest.mark.parametrize("a,b", ((2, 1), (1, 2)))
def test_timescale(torch_cuda, a, b):
    import solo_amd
    torch = torch_cuda
    M = geometry(16000, L, a, b)["M"]

    def make():
        h = handle()
        ins = dict(x=G.zeros(torch, (N, a, L), torch.int16))
        outs = dict(y=G.zeros(torch, (N, b, L), torch.int16), shift=G.zeros(torch, (N, M), torch.int32), cost=G.zeros(torch, (N, M), torch.int32),
                    count=G.zeros(torch, (4,), torch.int32))
        call = lambda: h.lib.solo_timescale(h.h, ins["x"].data_ptr(), N, a, b, outs["y"].data_ptr(), outs["shift"].data_ptr(), outs["cost"].data_ptr(),
                                            outs["count"].data_ptr(), h._stream())
        return G.Stage(torch, ins, outs, call, keep=h)

    def model(k, feed, got):
        want = model_timescale(feed["x"], b, 16000)
        assert np.array_equal(got["y"], want["out"]) and np.array_equal(got["shift"], want["shift"]) and np.array_equal(got["cost"], want["cost"]), k
        assert count_of(solo_amd.solo_timescale_count_t, got["count"]) == want["count"], k

    G.replay_against_twin(torch, make, [dict(x=timescale_rows(70 + 10 * a + k, N, 16000, L, a, b)[0]) for k in range(4)], model=model)


def _floor(k, P):
    """the inputs of a mixing call: 8 rows in 3 rooms (one row in none), loud enough to saturate, other rooms and gains for every k"""
    rng = np.random.default_rng(900 + k)
    pcm = (rng.integers(-32768, 32768, (N, P, L)) >> rng.integers(0, 6, (N, P, 1))).astype(np.int16)
    room = rng.permutation(np.array([0, 0, 0, 0, 1, 1, 2, -1], np.int32))
    gain = rng.integers(0, 8192, N).astype(np.int16)
    gain[rng.integers(0, N)] = -5
    return pcm, room, gain


def _mix_bufs(torch, P):
    return dict(pcm=G.zeros(torch, (N, P, L), torch.int16), room=G.zeros(torch, (N,), torch.int32), gain=G.zeros(torch, (N,), torch.int16))


def _shared_outs(torch, P):
    return dict(pcm_spk=G.zeros(torch, (N, P, L), torch.int16), spk_list=G.zeros(torch, (N,), torch.int32), spk_rows=G.zeros(torch, (N,), torch.int32),
                pcm_room=G.zeros(torch, (3, P, L), torch.int16), room_list=G.zeros(torch, (3,), torch.int32), source=G.zeros(torch, (N,), torch.int32),
                energy=G.zeros(torch, (N, P), torch.int64))


def _fills(got, keys):
    return {k: np.full_like(got[k], np.frombuffer(bytes([G.FILL]) * got[k].dtype.itemsize, got[k].dtype)[0]) for k in keys}


@pytest.mark.parametrize("max_speakers", (0, 3))
def test_mix(torch_cuda, max_speakers):
    import solo_amd
    torch = torch_cuda
    P = 2

    def make():
        h = handle()
        ins = _mix_bufs(torch, P)
        outs = dict(out=G.zeros(torch, (N, P, L), torch.int16), energy=G.zeros(torch, (N, P), torch.int64), mixed=G.zeros(torch, (N, P), torch.uint8),
                    count=G.zeros(torch, (4,), torch.int32))
        call = lambda: h.lib.solo_mix(h.h, ins["pcm"].data_ptr(), N, P, ins["room"].data_ptr(), 3, ins["gain"].data_ptr(), max_speakers, outs["out"].data_ptr(),
                                      outs["energy"].data_ptr(), outs["mixed"].data_ptr(), outs["count"].data_ptr(), h._stream())
        return G.Stage(torch, ins, outs, call, keep=h)

    def model(k, feed, got):
        f = _fills(got, ("out", "energy", "mixed"))
        want = model_mix(feed["pcm"], feed["room"], 3, feed["gain"], max_speakers, out=f["out"], energy=f["energy"], mixed=f["mixed"])
        assert all(np.array_equal(got[key], want[key]) for key in ("out", "energy", "mixed")), k
        assert count_of(solo_amd.solo_mix_count_t, got["count"]) == want["count"], k

    G.replay_against_twin(torch, make, [dict(zip(("pcm", "room", "gain"), _floor(k, P))) for k in range(4)], model=model)


def test_mix_shared(torch_cuda):
    import solo_amd
    torch = torch_cuda
    P = 2
    slots = np.array([1, 2, 4, 7, 8, 11, 12, 15], np.int32)

    def make():
        h = handle()
        ins = dict(_mix_bufs(torch, P), keep=G.zeros(torch, (N,), torch.uint8), slots=G.zeros(torch, (N,), torch.int32))
        outs = dict(_shared_outs(torch, P), mixed=G.zeros(torch, (N, P), torch.uint8), count=G.zeros(torch, (6,), torch.int32))
        call = lambda: h.lib.solo_mix_shared(h.h, ins["pcm"].data_ptr(), N, P, ins["room"].data_ptr(), 3, ins["gain"].data_ptr(), 2, ins["keep"].data_ptr(),
                                             ins["slots"].data_ptr(), outs["pcm_spk"].data_ptr(), outs["spk_list"].data_ptr(), outs["spk_rows"].data_ptr(),
                                             outs["pcm_room"].data_ptr(), outs["room_list"].data_ptr(), outs["source"].data_ptr(), outs["energy"].data_ptr(),
                                             outs["mixed"].data_ptr(), outs["count"].data_ptr(), h._stream())
        return G.Stage(torch, ins, outs, call, keep=h)

    def model(k, feed, got):
        keys = [key for key in got if key != "count"]
        want = model_mix_shared(feed["pcm"], feed["room"], 3, feed["gain"], 2, feed["keep"], feed["slots"], fill=_fills(got, keys))
        for key in keys:
            assert np.array_equal(got[key], want[key]), (k, key)
        assert count_of(solo_amd.solo_mix_shared_count_t, got["count"]) == want["count"], k

    feeds = []
    for k in range(4):
        pcm, room, gain = _floor(k, P)
        feeds.append(dict(pcm=pcm, room=room, gain=gain, keep=(np.arange(N) == k).astype(np.uint8), slots=slots + k))
    G.replay_against_twin(torch, make, feeds, model=model)


def test_mix_selected(torch_cuda):
    import solo_amd
    torch = torch_cuda
    P = 2

    def make():
        h = handle()
        ins = dict(_mix_bufs(torch, P), sel=G.zeros(torch, (N, P), torch.uint8), keep=G.zeros(torch, (N,), torch.uint8))
        outs = dict(_shared_outs(torch, P), room_nsel=G.zeros(torch, (3, P), torch.uint8), count=G.zeros(torch, (8,), torch.int32))
        call = lambda: h.lib.solo_mix_selected(h.h, ins["pcm"].data_ptr(), N, P, ins["room"].data_ptr(), 3, ins["gain"].data_ptr(), ins["sel"].data_ptr(),
                                               ins["keep"].data_ptr(), None, outs["pcm_spk"].data_ptr(), outs["spk_list"].data_ptr(), outs["spk_rows"].data_ptr(),
                                               outs["pcm_room"].data_ptr(), outs["room_list"].data_ptr(), outs["source"].data_ptr(), outs["room_nsel"].data_ptr(),
                                               outs["energy"].data_ptr(), outs["count"].data_ptr(), h._stream())
        return G.Stage(torch, ins, outs, call, keep=h)

    def model(k, feed, got):
        keys = [key for key in got if key != "count"]
        want = model_mix_selected(feed["pcm"], feed["room"], 3, feed["sel"], feed["gain"], feed["keep"], None, fill=_fills(got, keys))
        for key in keys:
            assert np.array_equal(got[key], want[key]), (k, key)
        assert count_of(solo_amd.solo_mix_selected_count_t, got["count"]) == want["count"], k

    feeds = []
    for k in range(4):
        pcm, room, gain = _floor(k, P)
        rng = np.random.default_rng(950 + k)
        feeds.append(dict(pcm=pcm, room=room, gain=gain, sel=(rng.integers(0, 3, (N, P)) == 0).astype(np.uint8) * 7, keep=(np.arange(N) == 7 - k).astype(np.uint8)))
    G.replay_against_twin(torch, make, feeds, model=model)


def _pack_inputs(k, P):
    """the fixture's packets [k P, (k + 1) P) and a send mask"""
    z = G.fixture()
    send = np.random.default_rng(300 + k).integers(0, 4, (N, P)).astype(np.uint8)
    return dict(bits=z["bits"][:, k * P:(k + 1) * P], nbytes=z["nbytes"][:, k * P:(k + 1) * P], send=send)


def _pack_stage(torch, h, P, list_rows, seq_base, first_seq):
    ins = dict(bits=G.zeros(torch, (N, P, SLOT), torch.uint8), nbytes=G.zeros(torch, (N, P, 2), torch.int16), send=G.zeros(torch, (N, P), torch.uint8))
    if seq_base:
        ins["seq_base"] = G.zeros(torch, (N,), torch.int32)
    if list_rows:
        ins["streams"] = G.zeros(torch, (N,), torch.int32)
    outs = dict(records=G.zeros(torch, (2 * N * P, 5), torch.int32), payload=G.zeros(torch, (N * P * SLOT,), torch.uint8), count=G.zeros(torch, (8,), torch.int32))
    tail = lambda: (ins["bits"].data_ptr(), ins["nbytes"].data_ptr(), ins["send"].data_ptr(), P, ptr(ins.get("seq_base")), first_seq, outs["records"].data_ptr(),
                    2 * N * P, outs["payload"].data_ptr(), N * P * SLOT, outs["count"].data_ptr(), h._stream())
    if list_rows:
        call = lambda: h.lib.solo_send_pack_streams(h.h, ins["streams"].data_ptr(), N, *tail())
    else:
        call = lambda: h.lib.solo_send_pack(h.h, *tail())
    return G.Stage(torch, ins, outs, call, keep=h)


def _pack_model(solo_amd, feed, got, seq_base, first_seq, streams=None):
    want = model_pack(feed["bits"], feed["nbytes"], feed["send"], seq_base, first_seq, 8, streams=streams)
    c = want["count"]
    assert count_of(solo_amd.solo_send_count_t, got["count"]) == c and c["records"] == c["records_needed"] > 0
    assert np.array_equal(got["records"][:c["records"]], want["records"]) and beyond(got["records"], c["records"], G.FILL32)
    assert np.array_equal(got["payload"][:c["bytes"]], want["payload"]) and beyond(got["payload"], c["bytes"], G.FILL)
    return want


def test_send_pack_device_sequence_base(torch_cuda):
    """d_seq_base lives on the device and is advanced there between replays: the sequence numbers move on"""
    import solo_amd
    torch = torch_cuda
    P = 2
    base0 = np.arange(N, dtype=np.int32) * 1000

    def between(stage, k):
        if k:
            stage.ins["seq_base"].add_(P)                    # (on the device, in place: the graph reads the same address)

    seen = []

    def model(k, feed, got):
        want = _pack_model(solo_amd, feed, got, base0 + k * P, 5)
        seen.append(set(want["records"][:, 1].tolist()))

    feeds = [dict(_pack_inputs(k, P), **(dict(seq_base=base0) if k == 0 else {})) for k in range(4)]
    G.replay_against_twin(torch, lambda: _pack_stage(torch, handle(), P, False, True, 5), feeds, model=model, between=between)
    assert all(not (seen[i] & seen[j]) for i in range(4) for j in range(i))


def test_send_pack_scalar_first_seq_repeats(torch_cuda):
    """first_seq is a host scalar: the capture freezes it, so every replay numbers its packets like the captured call (as documented:
    a tick that moves on brings d_seq_base)"""
    import solo_amd
    torch = torch_cuda
    P = 2
    seen = []

    def model(k, feed, got):
        want = _pack_model(solo_amd, feed, got, None, 100)
        seen.append(set(want["records"][:, 1].tolist()))

    G.replay_against_twin(torch, lambda: _pack_stage(torch, handle(), P, False, False, 100), [_pack_inputs(k, P) for k in range(4)], model=model)
    assert all(s == {100, 101} for s in seen)


def test_send_pack_streams(torch_cuda):
    """the rows' stream numbers are a device list of a handle of 16: other contents at every replay, the same length"""
    import solo_amd
    torch = torch_cuda
    P = 1
    lists = [np.sort(np.random.default_rng(40 + k).permutation(16)[:N]).astype(np.int32) for k in range(4)]
    assert len({tuple(l.tolist()) for l in lists}) == 4
    base0 = np.full(N, 7, np.int32)

    def model(k, feed, got):
        _pack_model(solo_amd, feed, got, base0, 0, streams=feed["streams"])

    make = lambda: _pack_stage(torch, solo_amd.SoloBatch(16, encoder=False, slot_bytes=SLOT), P, True, True, 0)
    G.replay_against_twin(torch, make, [dict(_pack_inputs(k, P), streams=lists[k], seq_base=base0) for k in range(4)], model=model)


def test_send_fanout(torch_cuda):
    import solo_amd
    torch = torch_cuda
    P, n_src, n_dst = 2, 8, 12

    def make():
        h = handle()
        ins = dict(bits=G.zeros(torch, (n_src, P, SLOT), torch.uint8), nbytes=G.zeros(torch, (n_src, P, 2), torch.int16), source=G.zeros(torch, (n_dst,), torch.int32),
                   dst_stream=G.zeros(torch, (n_dst,), torch.int32), send=G.zeros(torch, (n_dst, P), torch.uint8), seq_base=G.zeros(torch, (n_dst,), torch.int32))
        outs = dict(records=G.zeros(torch, (2 * n_dst * P, 5), torch.int32), payload=G.zeros(torch, (n_src * P * SLOT,), torch.uint8),
                    count=G.zeros(torch, (8,), torch.int32))
        call = lambda: h.lib.solo_send_fanout(h.h, ins["bits"].data_ptr(), ins["nbytes"].data_ptr(), n_src, ins["source"].data_ptr(), ins["dst_stream"].data_ptr(),
                                              n_dst, ins["send"].data_ptr(), P, ins["seq_base"].data_ptr(), 3, outs["records"].data_ptr(), 2 * n_dst * P,
                                              outs["payload"].data_ptr(), n_src * P * SLOT, outs["count"].data_ptr(), h._stream())
        return G.Stage(torch, ins, outs, call, keep=h)

    def model(k, feed, got):
        f = _fills(got, ("records", "payload"))
        want = model_fanout(feed["bits"], feed["nbytes"], feed["source"], 8, feed["dst_stream"], feed["send"], feed["seq_base"], 3, records=f["records"],
                            payload=f["payload"])
        assert np.array_equal(got["records"], want["records"]) and np.array_equal(got["payload"], want["payload"]), k
        assert count_of(solo_amd.solo_send_count_t, got["count"]) == want["count"] and want["count"]["records"] > 0, k

    keys = ("bits", "nbytes", "source", "dst_stream", "send", "seq_base")
    G.replay_against_twin(torch, make, [dict(zip(keys, fanout_case(60 + k, n_src, n_dst, P, SLOT, 8))) for k in range(4)], model=model)


# ---- the receiver ring: what the network brought is filed eagerly (or by the captured call), the ring call under test is the graph --------
DEPTH, RSLOT = 8, 256


def _ring_handle(torch, track=True):
    h = handle(decoder=True)
    h.recv_create(DEPTH, RSLOT, 0)
    if track:
        h.recv_track(True)
    h.payload = dev(torch, G.datagrams()[0])
    return h


def _records(pairs, seq_of=None):
    """the arrivals of these (stream, packet) pairs, at least one record (of stream -1 when nothing arrived)"""
    a, n = G.arrivals(pairs, max(2 * len(pairs), 1), seq_of)
    return a[:max(n, 1)]


def _file(torch, h, pairs, seq_of=None):
    h.recv_insert(dev(torch, _records(pairs, seq_of)), h.payload)


def _stats(h):
    out = (C.c_uint32 * 8)()
    assert h.lib.solo_recv_stats(h.h, out, h._stream()) == 0
    return [int(v) for v in out][:5]


def test_recv_report_with_a_play_list(torch_cuda):
    """four of the eight streams are reported per call, other ones at every replay; between the calls arrivals are filed and the
    selected streams of the call before are played, so queues, counters and margins all move; CLEAR_MARGIN makes the call stateful"""
    import solo_amd
    torch = torch_cuda
    lists = [[0, 2, 4, 6], [1, 2, 5, 7], [0, 3, 4, 7], [2, 3, 5, 6]]
    m = RingModel(N, DEPTH, RSLOT)
    m.track(True)
    # stream s has the packets [0, 1 + (s + k) % 3) of tick k filed ahead of the call; whoever was selected is then played one packet
    filed = {s: 0 for s in range(N)}
    plan = []
    for k in range(4):
        pairs = []
        for s in range(N):
            upto = min(filed[s] + (s + k) % 3, m.play[s] + DEPTH - 1) if k else 1 + s % 2
            pairs += [(s, p) for p in range(filed[s], upto)]
            filed[s] = max(filed[s], upto)
        plan.append(pairs)
    played = {}

    def between(stage, k):
        h = stage.keep
        if k and played[k - 1]:
            pcm = G.zeros(torch, (len(played[k - 1]), 1, L), torch.int16)
            assert h.lib.solo_recv_decode_streams(h.h, dev(torch, np.array(played[k - 1], np.int32)).data_ptr(), len(played[k - 1]), 1, pcm.data_ptr(), None,
                                                  h._stream()) == 0
        _file(torch, h, plan[k])

    def make():
        h = _ring_handle(torch)
        ins = dict(streams=G.zeros(torch, (4,), torch.int32))
        outs = dict(reports=G.zeros(torch, (4, 16), torch.int32), play_list=G.zeros(torch, (4,), torch.int32), play_rows=G.zeros(torch, (4,), torch.int32),
                    count=G.zeros(torch, (2,), torch.int32))
        call = lambda: h.lib.solo_recv_report(h.h, ins["streams"].data_ptr(), 4, None, 2, 0, solo_amd.RECV_REPORT_CLEAR_MARGIN, outs["reports"].data_ptr(),
                                              outs["play_list"].data_ptr(), outs["play_rows"].data_ptr(), outs["count"].data_ptr(), h._stream())
        return G.Stage(torch, ins, outs, call, keep=h)

    def model(k, feed, got):
        if k and played[k - 1]:
            m.play_out(played[k - 1])
        m.insert([tuple(int(v) for v in r) for r in _records(plan[k])], len(G.datagrams()[0]), [0] * N, {})
        rep, lst, rows = m.report(lists[k], min_ready=2, clear_margin=True)
        played[k] = lst
        assert got["count"].tolist() == [len(lst), 4], k
        assert np.array_equal(got["reports"].view(np.uint32), (rep % 2 ** 32).astype(np.uint32)), k
        assert got["play_list"][:len(lst)].tolist() == lst and got["play_rows"][:len(lst)].tolist() == rows, k
        assert beyond(got["play_list"], len(lst), G.FILL32) and beyond(got["play_rows"], len(lst), G.FILL32)

    # (the model runs inside replay_against_twin AFTER the calls of step k, and between() of step k + 1 needs played[k]: the model's
    # play list is computed ahead, from a model of its own)
    m2 = RingModel(N, DEPTH, RSLOT)
    m2.track(True)
    for k in range(4):
        if k and played[k - 1]:
            m2.play_out(played[k - 1])
        m2.insert([tuple(int(v) for v in r) for r in _records(plan[k])], len(G.datagrams()[0]), [0] * N, {})
        played[k] = m2.report(lists[k], min_ready=2, clear_margin=True)[1]
    assert any(played.values()) and any(len(v) < 4 for v in played.values())
    G.replay_against_twin(torch, make, [dict(streams=np.array(l, np.int32)) for l in lists], model=model, between=between)


def test_recv_insert_fixed_capacity(torch_cuda):
    """the captured call files A = 16 records; a tick that brought fewer pads with stream = -1, which is counted `bad` and nothing
    else: the handle's five counters are exact after every replay, and so are the queues (a report of all streams)"""
    torch = torch_cuda
    A = 2 * N
    m = RingModel(N, DEPTH, RSLOT)
    m.track(True)
    # call k: packet k of the streams (s + k) % 3 != 0, a second copy of packet k - 1 of stream 1, and packet k + DEPTH of stream 2
    feeds, want_stats = [], []
    for k in range(4):
        pairs = [(s, k) for s in range(N) if (s + k) % 3] + ([(1, k - 1)] if k else [])
        a, n = G.arrivals(pairs, A)
        far, _ = G.arrivals([(2, k)], 2, seq_of={(2, k): k + DEPTH})
        a[n:n + 1] = far[:1]
        feeds.append(dict(arrivals=a))
        m.insert([tuple(int(v) for v in r) for r in a], len(G.datagrams()[0]), [0] * N, {})
        want_stats.append(list(m.stats))
    assert want_stats[-1][4] > 0 and want_stats[-1][3] > 0 and want_stats[-1][2] > 0 and all(a[0] < b[0] for a, b in zip(want_stats, want_stats[1:]))

    def make():
        h = _ring_handle(torch)
        ins = dict(arrivals=G.zeros(torch, (A, 5), torch.int32))
        rep = G.zeros(torch, (N, 16), torch.int32)
        cnt = G.zeros(torch, (2,), torch.int32)

        def state():
            assert h.lib.solo_recv_report(h.h, None, N, None, 1, 0, 0, rep.data_ptr(), None, None, cnt.data_ptr(), h._stream()) == 0
            return np.concatenate([host(torch, rep).ravel(), np.array(_stats(h), np.int32)])

        call = lambda: h.lib.solo_recv_insert(h.h, ins["arrivals"].data_ptr(), A, h.payload.data_ptr(), h.payload.numel(), h._stream())
        # (the call has no output buffer: what it did is read back through the report and the statistics, as `outs` of one word each)
        st = G.Stage(torch, ins, {}, call, state=state, keep=h)
        st.read = lambda: dict(state=state())
        return st

    def model(k, feed, got):
        assert got["state"][-5:].tolist() == want_stats[k], (k, got["state"][-5:].tolist(), want_stats[k])

    _, cap, _ = G.replay_against_twin(torch, make, feeds, model=model, stateful=True)
    rep = m.report()[0]
    assert np.array_equal(cap.state()[:-5].astype(np.int64).reshape(N, 16) % 2 ** 32, rep % 2 ** 32)


def test_recv_decode(torch_cuda):
    """solo_recv_decode of one packet, the arrivals of the next packet filed before every replay: the reference decoder's PCM"""
    torch = torch_cuda
    z = G.fixture()

    def between(stage, k):
        _file(torch, stage.keep, [(s, k) for s in range(N)])

    def make():
        h = _ring_handle(torch, track=False)
        outs = dict(pcm=G.zeros(torch, (N, 1, L), torch.int16), status=G.zeros(torch, (N,), torch.int32))
        call = lambda: h.lib.solo_recv_decode(h.h, 1, outs["pcm"].data_ptr(), outs["status"].data_ptr(), h._stream())
        return G.Stage(torch, {}, outs, call, keep=h)

    def model(k, feed, got):
        assert np.array_equal(got["pcm"][:, 0], z["dec_loss"][:, k]) and not got["status"].any(), k

    G.replay_against_twin(torch, make, [{}] * 5, model=model, between=between)


def test_recv_decode_streams(torch_cuda):
    """two lists of four streams take turns: a stream that was not listed plays its own next packet when its turn comes"""
    torch = torch_cuda
    z = G.fixture()
    lists = [[0, 2, 4, 6], [1, 3, 5, 7]]
    turn = lambda k: lists[k % 2]

    def make():
        h = _ring_handle(torch, track=False)
        _file(torch, h, [(s, p) for s in range(N) for p in range(2)])
        _file(torch, h, [(s, p) for s in range(N) for p in range(2, 4)])
        ins = dict(streams=G.zeros(torch, (4,), torch.int32))
        outs = dict(pcm=G.zeros(torch, (4, 1, L), torch.int16), status=G.zeros(torch, (4,), torch.int32))
        call = lambda: h.lib.solo_recv_decode_streams(h.h, ins["streams"].data_ptr(), 4, 1, outs["pcm"].data_ptr(), outs["status"].data_ptr(), h._stream())
        return G.Stage(torch, ins, outs, call, keep=h)

    def model(k, feed, got):
        assert np.array_equal(got["pcm"][:, 0], z["dec_loss"][turn(k), k // 2]) and not got["status"].any(), k

    G.replay_against_twin(torch, make, [dict(streams=np.array(turn(k), np.int32)) for k in range(8)], model=model)


# ---- play-out control: the plan and the render, each on its own ----------------------------------------------------------------------------
PO_L, PO_BLOCK = 320, 80
PO_P = PM.params(start_ready=2, max_span=7, window=8, tolerate=1, lo=1, hi=3, cooldown=3, cost_gate=30000)


def _po_state(torch, po):
    return lambda: host(torch, po.get_state())


def test_playout_plan(torch_cuda):
    """eight rows, one of each family of the report script, 26 ticks into their run (the model's records of that moment are set on the
    device): from there four ticks in a row give four different plans; the reports are rewritten before every replay"""
    import solo_amd
    torch = torch_cuda
    script, pick = PM.ReportScript(64, DEPTH, PO_P["window"], PO_P["max_span"], seed=3), [0, 9, 18, 27, 36, 45, 54, 63]
    rows = [PM.Row(PO_L) for _ in range(N)]
    for _ in range(26):
        PM.plan(rows, list(range(N)), script.tick()[pick], PO_P, DEPTH)
    blob = np.concatenate([PM.records(rows), PM.held_store(rows).view(np.uint8)], axis=1)
    reps = [script.tick()[pick] for _ in range(4)]

    def make():
        po = solo_amd.Playout(N, PO_L)
        po.set_state(dev(torch, blob))
        ins = dict(reports=G.zeros(torch, (N, 16), torch.int32))
        outs = dict(action=G.zeros(torch, (N,), torch.int32), one=G.zeros(torch, (N,), torch.int32), two=G.zeros(torch, (N,), torch.int32),
                    stretch_pos=G.zeros(torch, (N,), torch.int32), count=G.zeros(torch, (4,), torch.int32))
        p = po.params(**PO_P)
        call = lambda: po.lib.solo_playout_plan(po.h, ins["reports"].data_ptr(), None, N, DEPTH, C.byref(p), outs["action"].data_ptr(), outs["one"].data_ptr(),
                                                outs["two"].data_ptr(), outs["stretch_pos"].data_ptr(), outs["count"].data_ptr(), po._stream())
        return G.Stage(torch, ins, outs, call, state=_po_state(torch, po), keep=po)

    def model(k, feed, got):
        pl = PM.plan(rows, list(range(N)), reps[k], PO_P, DEPTH)
        c = pl["count"]
        assert dict(zip(("n_one", "n_two", "n_stretch", "listed"), got["count"].tolist())) == c, k
        assert got["action"].tolist() == pl["action"], k
        for key, n in (("one", c["n_one"]), ("two", c["n_two"]), ("stretch_pos", c["n_stretch"])):
            assert got[key][:n].tolist() == pl[key] and beyond(got[key], n, G.FILL32), (k, key)

    _, cap, _ = G.replay_against_twin(torch, make, [dict(reports=PL.reports_i32(r)) for r in reps], model=model, stateful=True)
    assert np.array_equal(cap.state()[:, :128], PM.records(rows))


def test_playout_render(torch_cuda):
    """crafted states and ONE eager plan give idle, normal, held, stretch, accel and forced rows; the render of that plan is captured
    (its three counts are host scalars) and replayed on new decoder and scaler outputs: cum, cool and the held packets move on"""
    import solo_amd
    torch = torch_cuda
    rng = np.random.RandomState(5)
    rows, rep = PL.crafted_rows(PO_L, N, PO_P, rng)
    blob = np.concatenate([PM.records(rows), PM.held_store(rows).view(np.uint8)], axis=1)
    pl = PM.plan(rows, list(range(N)), rep, PO_P, DEPTH)
    c = pl["count"]
    assert sorted(set(pl["action"])) == list(range(6)) and min(c["n_one"], c["n_two"], c["n_stretch"]) > 0
    M = PO_L // PO_BLOCK
    decs = [PM.fake_decodes(rng, pl, PO_L, M) for _ in range(4)]
    keys = ("pcm_one", "st_one", "pcm_two", "st_two", "ts_s", "cost_s", "ts_a", "cost_a")

    def make():
        po = solo_amd.Playout(N, PO_L)
        po.set_state(dev(torch, blob))
        action = G.zeros(torch, (N,), torch.int32)
        side = [G.zeros(torch, (N,), torch.int32) for _ in range(4)]
        p = po.params(**PO_P)
        assert po.lib.solo_playout_plan(po.h, dev(torch, PL.reports_i32(rep)).data_ptr(), None, N, DEPTH, C.byref(p), action.data_ptr(), side[0].data_ptr(),
                                        side[1].data_ptr(), side[2].data_ptr(), side[3].data_ptr(), po._stream()) == 0
        assert host(torch, action).tolist() == pl["action"]
        ins = {k: dev(torch, decs[0][k]) for k in keys}
        outs = dict(heard=G.zeros(torch, (N, PO_L), torch.int16), outcome=G.zeros(torch, (N,), torch.int32), status=G.zeros(torch, (N,), torch.int32),
                    count=G.zeros(torch, (8,), torch.int32))
        call = lambda: po.lib.solo_playout_render(po.h, None, N, C.byref(p), PO_BLOCK, action.data_ptr(), c["n_one"], c["n_two"], c["n_stretch"],
                                                  *[ins[k].data_ptr() for k in keys], outs["heard"].data_ptr(), outs["outcome"].data_ptr(),
                                                  outs["status"].data_ptr(), outs["count"].data_ptr(), po._stream())
        return G.Stage(torch, ins, outs, call, state=_po_state(torch, po), keep=(po, action, side))

    def model(k, feed, got):
        heard, outcome, status, count = PM.render(rows, list(range(N)), pl, PO_P, **decs[k])
        assert np.array_equal(got["heard"], heard) and np.array_equal(got["outcome"], outcome) and np.array_equal(got["status"], status), k
        assert dict(zip(PM.OUTCOMES, got["count"].tolist())) == count, k

    _, cap, _ = G.replay_against_twin(torch, make, decs, model=model, stateful=True)
    st = cap.state()
    assert np.array_equal(st[:, :128], PM.records(rows)) and np.array_equal(st[:, 128:].view(np.int16), PM.held_store(rows))


# ==== 2. the codec calls ========================================================================================================================
def _assert_packets(bits, nb, ref_bits, ref_nb, what):
    """every byte count and every payload byte of the reference"""
    assert np.array_equal(nb, ref_nb), what
    for i in range(bits.shape[0]):
        for p in range(bits.shape[1]):
            n = int(nb[i, p, 0])
            assert np.array_equal(bits[i, p, :n], ref_bits[i, p, :n]), (what, i, p)


class Enc:
    """an encoder handle with its buffers allocated once: call() encodes what `pcm` holds into `bits` / `nbytes` / `status`"""

    def __init__(self, torch, P, n=N, n_streams=N, listed=False, samples=L, **kw):
        import solo_amd
        self.t, self.P = torch, P
        self.h = solo_amd.SoloBatch(n_streams, encoder=True, decoder=False, slot_bytes=SLOT, **kw)
        self.pcm = G.zeros(torch, (n, P, samples), torch.int16)
        self.bits, self.nb, self.status = G.zeros(torch, (n, P, SLOT), torch.uint8), G.zeros(torch, (n, P, 2), torch.int16), G.zeros(torch, (n,), torch.int32)
        self.streams = G.zeros(torch, (n,), torch.int32) if listed else None
        self.n = n

    def call(self):
        h = self.h
        if self.streams is not None:
            return h.lib.solo_batch_encode_streams(h.h, self.streams.data_ptr(), self.n, self.pcm.data_ptr(), self.P, self.bits.data_ptr(), self.nb.data_ptr(),
                                                   self.status.data_ptr(), h._stream())
        return h.lib.solo_batch_encode(h.h, self.pcm.data_ptr(), self.P, self.bits.data_ptr(), self.nb.data_ptr(), self.status.data_ptr(), h._stream())

    def put(self, pcm, streams=None):
        self.pcm.copy_(self.t.from_numpy(np.ascontiguousarray(pcm)))
        if streams is not None:
            self.streams.copy_(self.t.from_numpy(np.asarray(streams, np.int32)))
        for x in (self.bits, self.nb, self.status):
            x.view(self.t.uint8).fill_(G.FILL)

    def check(self, ref_bits, ref_nb, what):
        self.t.cuda.synchronize()
        assert not self.status.cpu().numpy().any(), what
        _assert_packets(self.bits.cpu().numpy(), self.nb.cpu().numpy(), ref_bits, ref_nb, what)


@pytest.mark.parametrize("P", (1, 3))
def test_encode(torch_cuda, P):
    """replay k encodes the fixture's packets [k P, (k + 1) P): the reference's bytes.  P = 3 is three chunks on the handle's three
    internal streams: a graph with parallel branches"""
    G.need_four_queues()
    torch, z = torch_cuda, G.fixture()
    e = Enc(torch, P)
    e.put(z["pcm"][:, :P])
    assert e.call() == 0                                    # the handle's first encode: set-up, scratch
    e.check(z["bits"][:, :P], z["nbytes"][:, :P], "eager")
    e.h.reset()
    graph = G.capture(torch, e.call)
    assert e.h.last_encode_chunks() == P
    outs = []
    for k in range(8):
        e.put(z["pcm"][:, k * P:(k + 1) * P])
        graph.replay()
        e.check(z["bits"][:, k * P:(k + 1) * P], z["nbytes"][:, k * P:(k + 1) * P], k)
        outs.append(dict(bits=e.bits.cpu().numpy()))
    assert G.differ(outs)
    # behind the replays, eagerly: a reset (it has to get past the join events the capture recorded) and the fixture from its start
    e.h.reset()
    e.put(z["pcm"][:, :P])
    assert e.call() == 0
    e.check(z["bits"][:, :P], z["nbytes"][:, :P], "eager, after the replays")


def test_encode_async_join(torch_cuda):
    """asynchronous joins: the capture holds the encode call and the solo_batch_wait_encode that joins its streams"""
    G.need_four_queues()
    torch, z = torch_cuda, G.fixture()
    P = 2
    e = Enc(torch, P)
    e.h.set_async_join(True)

    def call():
        h = e.h
        return [e.call(), h.lib.solo_batch_wait_encode(h.h, h._stream(), 0)]

    e.put(z["pcm"][:, :P])
    assert call() == [0, 0]
    e.check(z["bits"][:, :P], z["nbytes"][:, :P], "eager")
    e.h.reset()
    graph = G.capture(torch, call)
    for k in range(6):
        e.put(z["pcm"][:, k * P:(k + 1) * P])
        graph.replay()
        e.check(z["bits"][:, k * P:(k + 1) * P], z["nbytes"][:, k * P:(k + 1) * P], k)
    # behind the replays, eagerly: the wait for the latest call (recorded in the capture: the stream is the order), then two calls in flight
    assert e.h.lib.solo_batch_wait_encode(e.h.h, e.h._stream(), 0) == 0
    e.put(z["pcm"][:, 12:14])
    assert call() == [0, 0]
    e.check(z["bits"][:, 12:14], z["nbytes"][:, 12:14], "eager, after the replays")


LISTS = ([0, 2, 4, 6], [1, 3, 5, 7])


def test_encode_streams(torch_cuda):
    """two lists of four streams take turns, two packets a call: the unlisted streams go on from their own state when their turn
    comes.  Through the binding, which takes the device list as it is while a capture runs"""
    G.need_four_queues()
    torch, z = torch_cuda, G.fixture()
    P = 2
    e = Enc(torch, P, n=4, listed=True)
    call = lambda: e.h.encode(e.pcm, bits=e.bits, nbytes=e.nb, status=e.status, streams=e.streams) and 0
    e.put(z["pcm"][LISTS[0], :P], LISTS[0])
    assert call() == 0
    e.check(z["bits"][LISTS[0], :P], z["nbytes"][LISTS[0], :P], "eager")
    e.h.reset()
    graph = G.capture(torch, call)
    for k in range(8):
        rows, p0 = LISTS[k % 2], (k // 2) * P
        e.put(z["pcm"][rows, p0:p0 + P], rows)
        graph.replay()
        e.check(z["bits"][rows, p0:p0 + P], z["nbytes"][rows, p0:p0 + P], k)
    # outside a capture the binding still reads the list and refuses a bad one on the host
    with pytest.raises(ValueError):
        e.h.encode(e.pcm, streams=dev(torch, np.array([0, 2, 2, 6], np.int32)))


def test_encode_32k(torch_cuda):
    """the 32 kHz mode, four streams of tests/golden/enc_stages_wb.npz (one at the upper rate clamp), two packets a replay"""
    G.need_four_queues()
    torch = torch_cuda
    z = np.load(T.GOLDEN + "/enc_stages_wb.npz")
    n, P = int(z["n_streams"]), 2
    prm = np.stack([z["s%02d_params" % i] for i in range(n)])
    assert n == 4 and (prm[:, 0] == 32000).all() and not prm[:, 2:5].any() and (prm[:, 5] == 40).all() and (prm[:, 6] == 16).all()
    pcm = np.stack([z["s%02d_pcm" % i] for i in range(n)])
    ref_nb = np.stack([z["s%02d_nbytes" % i] for i in range(n)])
    ref_bits = np.zeros((n, 16, SLOT), np.uint8)
    for i in range(n):
        b = z["s%02d_bits" % i]
        ref_bits[i, :, :b.shape[1]] = b
    rates = [int(r) for r in prm[:, 1]]
    e = Enc(torch, P, n=n, n_streams=n, samples=1280, rate=24000, samplerate=32000)
    e.h.reset_streams(list(range(n)), rate=rates, which="enc")
    e.put(pcm[:, :P])
    assert e.call() == 0
    e.check(ref_bits[:, :P], ref_nb[:, :P], "eager")
    e.h.reset_streams(list(range(n)), rate=rates, which="enc")
    graph = G.capture(torch, e.call)
    for k in range(8):
        e.put(pcm[:, k * P:(k + 1) * P])
        graph.replay()
        e.check(ref_bits[:, k * P:(k + 1) * P], ref_nb[:, k * P:(k + 1) * P], k)


class Dec:
    """a decoder handle with its buffers allocated once; kind: "batch", "streams" (a device list of four) or "split" (arrival slots)"""

    def __init__(self, torch, P, kind="batch"):
        import solo_amd
        self.t, self.P, self.kind = torch, P, kind
        n = self.n = 4 if kind == "streams" else N
        self.h = solo_amd.SoloBatch(N, encoder=False, decoder=True, slot_bytes=SLOT)
        self.bits, self.nb, self.recv = G.zeros(torch, (n, P, SLOT), torch.uint8), G.zeros(torch, (n, P, 2), torch.int16), G.zeros(torch, (n, P), torch.uint8)
        self.pcm, self.status = G.zeros(torch, (n, P, L), torch.int16), G.zeros(torch, (n,), torch.int32)
        self.streams = G.zeros(torch, (n,), torch.int32)
        self.S = 256
        self.dA, self.dB = G.zeros(torch, (n, P, self.S), torch.uint8), G.zeros(torch, (n, P, self.S), torch.uint8)
        self.lA, self.lB = G.zeros(torch, (n, P), torch.int16), G.zeros(torch, (n, P), torch.int16)

    def call(self):
        h, st = self.h, self.h._stream()
        if self.kind == "split":
            return h.lib.solo_batch_decode_split(h.h, self.dA.data_ptr(), self.lA.data_ptr(), self.dB.data_ptr(), self.lB.data_ptr(), self.S, self.P,
                                                 self.pcm.data_ptr(), self.status.data_ptr(), st)
        if self.kind == "streams":
            return h.lib.solo_batch_decode_streams(h.h, self.streams.data_ptr(), self.n, self.bits.data_ptr(), self.nb.data_ptr(), self.recv.data_ptr(), self.P,
                                                   self.pcm.data_ptr(), self.status.data_ptr(), st)
        return h.lib.solo_batch_decode(h.h, self.bits.data_ptr(), self.nb.data_ptr(), self.recv.data_ptr(), self.P, self.pcm.data_ptr(), self.status.data_ptr(), st)

    def put(self, rows, p0, P=None):
        """the fixture's packets [p0, p0 + P) of `rows` into the static inputs"""
        z, t = G.fixture(), self.t
        P = self.P if P is None else P
        up = lambda dst, a: dst.copy_(t.from_numpy(np.ascontiguousarray(a)))
        bits, nb, recv = z["bits"][rows, p0:p0 + P], z["nbytes"][rows, p0:p0 + P], z["recv"][rows, p0:p0 + P]
        if self.kind == "split":
            dA, dB = np.zeros((self.n, P, self.S), np.uint8), np.zeros((self.n, P, self.S), np.uint8)
            lA, lB = np.zeros((self.n, P), np.int16), np.zeros((self.n, P), np.int16)
            for i in range(self.n):
                for p in range(P):
                    n0, n1 = int(nb[i, p, 0]), int(nb[i, p, 1])
                    if recv[i, p] & 1:
                        dA[i, p, :n0 - n1], lA[i, p] = bits[i, p, :n0 - n1], n0 - n1
                    if recv[i, p] & 2:
                        dB[i, p, :n1], lB[i, p] = bits[i, p, n0 - n1:n0], n1
            up(self.dA, dA), up(self.lA, lA), up(self.dB, dB), up(self.lB, lB)
        else:
            up(self.bits, bits), up(self.nb, nb), up(self.recv, recv)
        up(self.streams, np.asarray(rows, np.int32))
        for x in (self.pcm, self.status):
            x.view(t.uint8).fill_(G.FILL)

    def check(self, rows, p0, what, P=None):
        P = self.P if P is None else P
        self.t.cuda.synchronize()
        assert not self.status.cpu().numpy().any(), what
        assert np.array_equal(self.pcm.cpu().numpy()[:, :P], G.fixture()["dec_loss"][rows, p0:p0 + P]), what


def _decode(torch, kind, P):
    d, rows = Dec(torch, P, kind), list(range(N))
    d.put(rows, 0)
    assert d.call() == 0                                    # the handle's first decode: set-up, the buffer of extraction records
    d.check(rows, 0, "eager")
    d.h.reset()
    graph = G.capture(torch, d.call)
    outs = []
    for k in range(8):
        d.put(rows, k * P)
        graph.replay()
        d.check(rows, k * P, k)
        outs.append(dict(pcm=d.pcm.cpu().numpy()))
    assert G.differ(outs)


@pytest.mark.parametrize("P", (1, 3))
def test_decode(torch_cuda, P):
    """replay k decodes the fixture's packets [k P, (k + 1) P) under its loss mask: the reference decoder's PCM"""
    _decode(torch_cuda, "batch", P)


def test_decode_split(torch_cuda):
    """the same through the arrival slots A and B, built from the fixture under its loss mask"""
    _decode(torch_cuda, "split", 2)


def test_decode_streams(torch_cuda):
    """two lists of four streams take turns, two packets a call"""
    torch = torch_cuda
    P = 2
    d = Dec(torch, P, "streams")
    d.put(LISTS[0], 0)
    assert d.call() == 0
    d.check(LISTS[0], 0, "eager")
    d.h.reset()
    graph = G.capture(torch, d.call)
    for k in range(8):
        rows, p0 = LISTS[k % 2], (k // 2) * P
        d.put(rows, p0)
        graph.replay()
        d.check(rows, p0, k)


# ==== 3. eager calls and replays interleaved on one handle =========================================================================================
def _interleaved(torch, x, eager_first, side_stream=False):
    """x: an Enc or a Dec of P = 3 (its buffers take calls of 1, 2 and 3 packets).  Eager calls of 3 and of 2 packets and a reset first:
    the set-up and the largest scratch the run will need (a graph holds the scratch's address).  Then, along the fixture's 25 packets:
    `eager_first` eager calls of one packet, the capture of a call of two, two replays, an eager call of THREE packets (another layout of
    the hand-over records: it waits for everything of the call before it, which ran inside a graph), a replay, eager calls of one packet
    to the end.  -> the (first packet, packets) of every call in order"""
    z = G.fixture()
    rows = list(range(N))
    is_enc = isinstance(x, Enc)

    def run(p0, P, how):
        if is_enc:
            x.P = P
            buf = np.zeros(N * 3 * L, np.int16)
            buf[:N * P * L] = z["pcm"][:, p0:p0 + P].ravel()      # (a call of P packets reads [N][P][L] from the front of the buffer)
            x.put(buf.reshape(N, 3, L))
        else:
            x.P = P
            _dec_put_front(x, rows, p0, P)
        how()
        torch.cuda.synchronize()
        if is_enc:
            assert not x.status.cpu().numpy().any(), (p0, P)
            bits = x.bits.cpu().numpy().ravel()[:N * P * SLOT].reshape(N, P, SLOT)
            nb = x.nb.cpu().numpy().ravel()[:N * P * 2].reshape(N, P, 2)
            _assert_packets(bits, nb, z["bits"][:, p0:p0 + P], z["nbytes"][:, p0:p0 + P], (p0, P))
        else:
            assert not x.status.cpu().numpy().any(), (p0, P)
            pcm = x.pcm.cpu().numpy().ravel()[:N * P * L].reshape(N, P, L)
            assert np.array_equal(pcm, z["dec_loss"][:, p0:p0 + P]), (p0, P)
        done.append((p0, P))

    def eager():
        assert x.call() == 0

    def eager_aside():
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            assert x.call() == 0
        torch.cuda.current_stream().wait_stream(s)

    done = []
    run(0, 3, eager)
    x.h.reset()
    run(0, 2, eager)
    x.h.reset()
    done.clear()
    at = 0
    for _ in range(eager_first):
        run(at, 1, eager)
        at += 1
    x.P = 2
    graph = G.capture(torch, x.call)
    for _ in range(2):
        run(at, 2, graph.replay)
        at += 2
    run(at, 3, eager_aside if side_stream else eager)
    at += 3
    run(at, 2, graph.replay)
    at += 2
    while at < 25:
        run(at, 1, eager)
        at += 1
    return done


def _dec_put_front(d, rows, p0, P):
    """the fixture's packets [p0, p0 + P) as a call of P packets at the front of the decoder's three-packet buffers"""
    z, t = G.fixture(), d.t
    for dst, a, w in ((d.bits, z["bits"], SLOT), (d.nb, z["nbytes"], 2), (d.recv, z["recv"][:, :, None], 1)):
        buf = np.zeros(N * 3 * w, a.dtype)
        buf[:N * P * w] = a[rows, p0:p0 + P].ravel()
        dst.copy_(t.from_numpy(buf).reshape(dst.shape))
    for x in (d.pcm, d.status):
        x.view(t.uint8).fill_(G.FILL)


@pytest.mark.parametrize("eager_first", (1, 2), ids=("odd", "even"))
def test_encode_interleaved(torch_cuda, eager_first):
    """the capture begins at an odd / an even number of encode calls: the call's join events and those it waits for change places"""
    G.need_four_queues()
    done = _interleaved(torch_cuda, Enc(torch_cuda, 3), eager_first)
    assert sum(P for _, P in done) == 25 and [P for _, P in done][eager_first:eager_first + 4] == [2, 2, 3, 2]


def test_decode_interleaved(torch_cuda):
    """the eager decode after the replays is issued on another torch stream than they were"""
    done = _interleaved(torch_cuda, Dec(torch_cuda, 3), 1, side_stream=True)
    assert sum(P for _, P in done) == 25 and [P for _, P in done][1:5] == [2, 2, 3, 2]


def test_decode_grows_after_a_capture(torch_cuda):
    """a call larger than every one before, issued after a capture: the buffer of extraction records grows (the one place where the
    library synchronises with the event a decode call leaves, here last recorded inside a capture).  The graph captured before holds the
    old buffer's address and is dropped; a new one is captured at the new size"""
    torch, z = torch_cuda, G.fixture()
    d, rows = Dec(torch, 3), list(range(N))

    def run(p0, P, how):
        d.P = P
        _dec_put_front(d, rows, p0, P)
        how()
        torch.cuda.synchronize()
        assert not d.status.cpu().numpy().any(), (p0, P)
        assert np.array_equal(d.pcm.cpu().numpy().ravel()[:N * P * L].reshape(N, P, L), z["dec_loss"][:, p0:p0 + P]), (p0, P)

    def eager():
        assert d.call() == 0

    run(0, 1, eager)
    d.h.reset()
    d.P = 1
    graph = G.capture(torch, d.call)
    run(0, 1, graph.replay)
    run(1, 1, graph.replay)
    del graph
    run(2, 3, eager)                                        # grows
    d.P = 3
    graph = G.capture(torch, d.call)
    run(5, 3, graph.replay)
    run(8, 3, graph.replay)
    run(11, 1, eager)


# ==== 4. the bridge tick in one graph ===============================================================================================================
class Bridge:
    """8 slots in two rooms, six of them live per tick: rx handle with ring, Vad, Agc, tx handle, and every buffer of the tick allocated
    once.  Every live row keeps its own encoder (d_keep all ones: the caller's hangover policy at its longest), so the encode call has
    the live list's length, which the graph freezes; who is HEARD is solo_vad_select's choice, tick by tick."""
    A, NL = 2 * N, 6

    def __init__(self, torch):
        import solo_amd
        t, n, z = torch, self.NL, G.zeros
        self.t = torch
        self.rx, self.tx = _ring_handle(torch, track=False), solo_amd.SoloBatch(N, encoder=True, decoder=False, slot_bytes=SLOT)
        self.vad, self.agc = solo_amd.Vad(N, 320), solo_amd.Agc(N)
        self.ins = dict(arrivals=z(t, (self.A, 5), t.int32), live=z(t, (n,), t.int32), room=z(t, (n,), t.int32), seq=z(t, (n,), t.int32))
        self.ones = t.ones((n,), dtype=t.uint8, device="cuda")
        self.outs = dict(
            heard=z(t, (n, 1, L), t.int16), dec_status=z(t, (n,), t.int32), sa=z(t, (n, 1, 2), t.uint8), level=z(t, (n, 1), t.uint8), vad_count=z(t, (4,), t.int32),
            lev_pcm=z(t, (n, 1, L), t.int16), lev_level=z(t, (n, 1), t.uint8), gain_q8=z(t, (n, 1), t.int16), agc_count=z(t, (4,), t.int32),
            sel=z(t, (n, 1), t.uint8), gain_out=z(t, (n,), t.int16), keep=z(t, (n,), t.uint8), dominant=z(t, (2, 1), t.int32), sel_count=z(t, (4,), t.int32),
            pcm_spk=z(t, (n, 1, L), t.int16), spk_list=z(t, (n,), t.int32), spk_rows=z(t, (n,), t.int32), pcm_room=z(t, (2, 1, L), t.int16),
            room_list=z(t, (2,), t.int32), source=z(t, (n,), t.int32), room_nsel=z(t, (2, 1), t.uint8), mix_count=z(t, (8,), t.int32),
            bits=z(t, (n, 1, SLOT), t.uint8), nbytes=z(t, (n, 1, 2), t.int16), enc_status=z(t, (n,), t.int32),
            records=z(t, (2 * n, 5), t.int32), pool=z(t, (n * SLOT,), t.uint8), send_count=z(t, (8,), t.int32))
        self.sp = solo_amd.solo_vad_select_params_t(2, 128, 64, 2, 6)
        self.ap = solo_amd.solo_agc_params_t(*[int(v) for v in AM.params_words(up=512)])

    def tick(self):
        """the chain of INTEGRATION.md section 2 on the current stream -> the statuses"""
        i, o, n, rx, tx, v, g = self.ins, self.outs, self.NL, self.rx, self.tx, self.vad, self.agc
        st = rx._stream()
        p = lambda k: (i[k] if k in i else o[k]).data_ptr()
        return [
            rx.lib.solo_recv_insert(rx.h, p("arrivals"), self.A, rx.payload.data_ptr(), rx.payload.numel(), st),
            rx.lib.solo_recv_decode_streams(rx.h, p("live"), n, 1, p("heard"), p("dec_status"), st),
            v.lib.solo_vad(v.h, p("live"), n, p("heard"), 1, L, p("sa"), None, p("level"), p("vad_count"), st),
            g.lib.solo_agc(g.h, p("live"), n, p("heard"), 1, L, p("level"), p("sa"), 2, C.byref(self.ap), p("lev_pcm"), p("lev_level"), p("gain_q8"),
                           p("agc_count"), st),
            v.lib.solo_vad_select(v.h, p("live"), n, p("sa"), p("lev_level"), 1, 2, p("room"), 2, C.byref(self.sp), None, p("sel"), p("gain_out"), p("keep"),
                                  p("dominant"), p("sel_count"), st),
            rx.lib.solo_mix_selected(rx.h, p("lev_pcm"), n, 1, p("room"), 2, None, p("sel"), self.ones.data_ptr(), p("live"), p("pcm_spk"), p("spk_list"),
                                     p("spk_rows"), p("pcm_room"), p("room_list"), p("source"), p("room_nsel"), None, p("mix_count"), st),
            tx.lib.solo_batch_encode_streams(tx.h, p("spk_list"), n, p("pcm_spk"), 1, p("bits"), p("nbytes"), p("enc_status"), st),
            tx.lib.solo_send_pack_streams(tx.h, p("spk_list"), n, p("bits"), p("nbytes"), None, 1, p("seq"), 0, p("records"), 2 * n, p("pool"), n * SLOT,
                                          p("send_count"), st),
        ]

    def put(self, feed):
        for k, a in feed.items():
            self.ins[k].copy_(self.t.from_numpy(np.ascontiguousarray(a)))
        for x in self.outs.values():
            x.view(self.t.uint8).fill_(G.FILL)

    def read(self):
        self.t.cuda.synchronize()
        out = {k: x.cpu().numpy() for k, x in self.outs.items()}
        out["vad_state"], out["agc_state"] = self.vad.get_state().cpu().numpy(), self.agc.get_state().cpu().numpy()
        return out


def test_bridge_tick_in_one_graph(torch_cuda):
    """one eager tick (set-up, scratch), the capture of the whole chain, six replays against twin handles that run the same ticks
    eagerly -- every output buffer of every stage of every tick, and the VAD and AGC states --, then two more eager ticks on both: the
    codec, ring, VAD and AGC state went through the replays intact"""
    G.need_four_queues()
    torch = torch_cuda
    lives = [sorted(np.random.default_rng(70 + k).permutation(N)[:Bridge.NL].tolist()) for k in range(9)]
    assert len({tuple(l) for l in lives[1:7]}) >= 4
    played = np.zeros(N, np.int64)
    feeds = []
    for k, live in enumerate(lives):
        # every live stream's next packet arrives (under the fixture's loss mask) under the sequence number the ring plays next
        a, n = G.arrivals([(s, int(played[s])) for s in live], Bridge.A)
        assert 0 < n < Bridge.A
        feeds.append(dict(arrivals=a, live=np.array(live, np.int32), room=np.array([s % 2 for s in live], np.int32), seq=played[live].astype(np.int32)))
        played[live] += 1
    cap, twin = Bridge(torch), Bridge(torch)
    for b in (cap, twin):
        b.put(feeds[0])
        assert not any(b.tick())
    assert G.same(cap.read(), twin.read())
    graph = G.capture(torch, cap.tick)
    outs = []
    for k in range(1, 9):
        cap.put(feeds[k])
        twin.put(feeds[k])
        if k < 7:
            graph.replay()
        else:
            assert not any(cap.tick())
        assert not any(twin.tick())
        got, want = cap.read(), twin.read()
        for name in got:
            assert np.array_equal(got[name], want[name]), (k, name)
        # the tick did what a tick does: every live row decoded, levelled, mixed, encoded and packed
        assert not got["dec_status"].any() and not got["enc_status"].any() and got["vad_count"][0] == Bridge.NL and got["mix_count"][0] == Bridge.NL
        assert got["spk_list"].tolist() == lives[k] and (got["nbytes"][:, 0, 0] > 0).all() and got["send_count"][0] > 0
        outs.append(got)
    assert G.differ(outs) and any(o["sel"].any() for o in outs)

"""What the graph tests (tests/test_gpu_graph_replay.py) share: a stage whose buffers are allocated once, the capture of one call of it,
and the comparison of its replays with the same calls issued eagerly on a twin.  No arithmetic lives here."""
import os

import numpy as np
import pytest

import solo_testlib as T

FILL = 0x5A                                                 # every output buffer starts each call from this byte
FILL16, FILL32 = 0x5A5A, 0x5A5A5A5A


def need_four_queues():
    """a captured encode is a graph with parallel branches: the HIP runtime is known to crash replaying one on fewer than 4 hardware
    queues, so such a test does not run where the environment asks for fewer"""
    v = os.environ.get("GPU_MAX_HW_QUEUES", "")
    if v.strip().lstrip("-").isdigit() and int(v) < 4:
        pytest.skip("GPU_MAX_HW_QUEUES=%s: a captured encode needs at least 4 hardware queues" % v)


class Stage:
    """one entry point with its objects and its buffers: `ins` and `outs` are dicts of CUDA tensors allocated once, call() issues the
    call on the current stream with their addresses and returns its status, state() (optional) returns the carried state as an array"""

    def __init__(self, torch, ins, outs, call, state=None, keep=None):
        self.torch, self.ins, self.outs, self.call, self.state, self.keep = torch, ins, outs, call, state, keep

    def put(self, feed):
        """rewrites the inputs in place"""
        for k, a in feed.items():
            a = np.ascontiguousarray(a)
            assert tuple(a.shape) == tuple(self.ins[k].shape) and str(a.dtype) == str(self.ins[k].dtype).split(".")[-1], k
            self.ins[k].copy_(self.torch.from_numpy(a))

    def fill(self):
        for t in self.outs.values():
            t.view(self.torch.uint8).fill_(FILL)

    def read(self):
        self.torch.cuda.synchronize()
        return {k: t.cpu().numpy() for k, t in self.outs.items()}


def zeros(torch, shape, dtype):
    return torch.zeros(shape, dtype=dtype, device="cuda")


def capture(torch, fn):
    """fn() issues library calls on the current stream and returns their statuses; captured with torch's default error mode"""
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    r = []
    try:
        with torch.cuda.graph(g):
            r.append(fn())
    except Exception as e:                                  # (what the call returned belongs in the report)
        raise AssertionError("the capture failed, the call returned %r: %s" % (r, e))
    assert r[0] == 0 or (isinstance(r[0], (list, tuple)) and not any(r[0])), r
    return g


def same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


def differ(outs):
    """every two of the replays gave different outputs"""
    return all(not same(outs[i], outs[j]) for i in range(len(outs)) for j in range(i))


def replay_against_twin(torch, make, feeds, model=None, between=None, stateful=False):
    """make() -> a Stage (called twice: the captured one and its twin).  feeds[0] is the eager call of the same geometry that both make
    first (one-time set-up, scratch growth); then ONE call of the first stage is captured and replayed len(feeds) - 1 times, its inputs
    rewritten in place before every replay, and every output buffer compared with the twin's, which makes the same calls eagerly.
    model(k, feed, got) compares replay k with the Python model; between(stage, k) runs on both ahead of call k (device-side changes
    of the inputs, eager calls that feed the stage).  The replays must differ from each other; with `stateful` the state is compared
    after the capture (a capture runs nothing) and at the end.  -> the outputs of the replays"""
    cap, twin = make(), make()
    for s in (cap, twin):
        if between:
            between(s, 0)
        s.put(feeds[0])
        s.fill()
        assert s.call() == 0
    warm = cap.read()
    assert same(warm, twin.read())
    if model:
        model(0, feeds[0], warm)
    before = cap.state() if stateful else None
    graph = capture(torch, cap.call)
    if stateful:
        assert np.array_equal(cap.state(), before) and np.array_equal(twin.state(), before)
    outs = []
    for k, feed in enumerate(feeds[1:], 1):
        for s in (cap, twin):
            if between:
                between(s, k)
            s.put(feed)
            s.fill()
        graph.replay()
        assert twin.call() == 0
        got, want = cap.read(), twin.read()
        for name in got:
            assert np.array_equal(got[name], want[name]), (k, name)
        if model:
            model(k, feed, got)
        outs.append(got)
    assert differ(outs)
    if stateful:
        st = cap.state()
        assert np.array_equal(st, twin.state()) and not np.array_equal(st, before)
    return outs, cap, twin


# ---- the codec fixture as datagrams -------------------------------------------------------------------------------------------------------
_fix = {}


def fixture():
    """tests/golden/synth8x25.npz: 8 streams x 25 packets, the reference's bitstreams and its decoder's PCM under the `recv` mask"""
    if "z" not in _fix:
        _fix["z"] = dict(np.load(os.path.join(T.GOLDEN, "synth8x25.npz")))
    return _fix["z"]


def datagrams():
    """the fixture's packets as the network carries them -> (pool uint8 [bytes], parts {(stream, packet, description): (offset, len)}):
    only the descriptions the fixture's `recv` mask lets through, so a ring fed from here plays what `dec_loss` holds"""
    if "pool" not in _fix:
        z = fixture()
        parts, blobs, off = {}, [], 0
        N, P = z["recv"].shape
        for s in range(N):
            for p in range(P):
                n0, n1 = int(z["nbytes"][s, p, 0]), int(z["nbytes"][s, p, 1])
                for d, (a, b) in enumerate(((0, n0 - n1), (n0 - n1, n0))):
                    if z["recv"][s, p] >> d & 1 and b > a:
                        parts[s, p, d] = (off, b - a)
                        blobs.append(z["bits"][s, p, a:b])
                        off += b - a
        _fix["pool"], _fix["parts"] = np.concatenate(blobs), parts
    return _fix["pool"], _fix["parts"]


def arrivals(pairs, capacity, seq_of=None):
    """pairs: (stream, packet) -> int32 [capacity, 5]: the arrivals of those packets (stream, seq, desc, offset, len), seq = the packet
    number or seq_of[stream, packet]; the unused records carry stream -1, which solo_recv_insert counts as `bad` and nothing else"""
    _, parts = datagrams()
    rows = [(s, p if seq_of is None else seq_of[s, p], d) + parts[s, p, d] for s, p in pairs for d in (0, 1) if (s, p, d) in parts]
    assert len(rows) <= capacity
    a = np.zeros((capacity, 5), np.int32)
    a[:, 0] = -1
    if rows:
        a[:len(rows)] = rows
    return a, len(rows)

"""The argument checks of the Python binding, every tensor-taking method of SoloBatch, Resampler and Vad from one table.

Negative half: from a valid argument set of a method, each tensor argument in turn is put on the host, given a wrong dtype, made
non-contiguous, given a dimension off by one or a dimension too many, or left out where it is required, and a streams= list is
given as a device tensor of a wrong dtype or rank; each must raise ValueError while NoLib stands in for the library, so nothing
reaches it.  Positive half: the valid set reaches a recording stand-in for the
library exactly as the prototype of load_library() orders it -- function name, integers and pointers, the pointers being made-up
addresses of the fakes, those of the outputs the call returns, or None for an absent optional.

A CPU test on purpose (no GPU variant): were a check wrong, the negative half on a device would hand a host pointer to a kernel."""
import ctypes as C
import itertools

import pytest

import solo_amd
import solo_testlib as T

torch = pytest.importorskip("torch")
I16, I32, I64, U8 = torch.int16, torch.int32, torch.int64, torch.uint8
N, P, L, SLOT, H = 8, 3, 640, 512, 0x5010        # the handle's streams / rows, packets of a call, packet samples, slot bytes, the handle
LIST = [1, 4, 6]                                 # a host list of streams: the binding copies it to the device itself ...
ANY = object()                                   # ... so its address is not one of the fakes'


class Dev(T.FakeDev):
    """a FakeDev the library stand-in can be handed: a made-up address of its own, and the CPU device for the default outputs"""
    _next = itertools.count(1)
    device = torch.device("cpu")

    def __init__(self, shape, dtype, cuda=True, contiguous=True):
        super().__init__(shape, dtype, cuda, contiguous)
        self._ptr = 0x1000 * next(Dev._next)

    def data_ptr(self):
        return self._ptr

    def dim(self):
        return len(self.shape)

    def numel(self):
        n = 1
        for d in self.shape:
            n *= d
        return n


class X:
    """a tensor argument of a table row: dtype, shape, the dimensions nothing else in the row pins (free), whether None is allowed
    (opt), whether the argument is "a sequence or a CUDA tensor" (seq: an object on the host is then a sequence, not a fault)"""

    def __init__(self, dtype, *shape, free=(), opt=False, seq=False):
        self.dtype, self.shape, self.free, self.opt, self.seq = dtype, shape, free, opt, seq

    def make(self, **kw):
        return Dev(kw.pop("shape", self.shape), kw.pop("dtype", self.dtype), **kw)

    def faults(self):
        out = {"dtype": self.make(dtype=torch.float32), "noncontiguous": self.make(contiguous=False), "rank": self.make(shape=self.shape + (1,))}
        if not self.seq:
            out["host"] = self.make(cuda=False)
        for d in range(len(self.shape)):
            if d not in self.free:
                out["dim%d" % d] = self.make(shape=self.shape[:d] + (self.shape[d] + 1,) + self.shape[d + 1:])
        if not self.opt:
            out["none"] = None
        return out


class Recorder:
    """stands in for the library: records every call (name, arguments as plain values) and returns 0"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name,) + tuple(_plain(a) for a in args))
            return 0
        return call


class NoLibBut(T.NoLib):
    """NoLib that answers the named queries (they enqueue nothing) with 0"""

    def __init__(self, queries):
        self.__dict__["_queries"] = queries

    def __getattr__(self, name):
        if name in self._queries:
            return lambda *args: 0
        return super().__getattr__(name)


def _plain(a):
    if isinstance(a, C.Array):
        return tuple(a)
    if hasattr(a, "_obj"):                       # byref(structure)
        return tuple(getattr(a._obj, f) for f, _ in a._obj._fields_)
    if isinstance(a, C.c_void_p):
        return a.value
    return a


def _object(kind, lib):
    if kind == "SoloBatch":
        o = object.__new__(solo_amd.SoloBatch)
        o.n_streams, o.slot, o.packet_samples, o.samplerate = N, SLOT, L, 16000
        o._enc = o._dec = object()
    elif kind == "Resampler":
        o = object.__new__(solo_amd.Resampler)
        o.n_rows, o.fs_in, o.fs_out = N, 48000, 16000
    else:
        o = object.__new__(solo_amd.Vad)
        o.n_rows, o.frame = N, 320
    o.torch, o.lib, o.h, o.device = torch, lib, H, torch.device("cpu")
    o._stream = lambda: None
    return o


def _call(row, kw, lib):
    o = _object(row["kind"], lib)
    try:
        return getattr(o, row["method"])(**kw)
    finally:
        o.h = None                               # (nothing to destroy)


def p(x):
    return None if x is None else x.data_ptr()


def row(kind, method, args, calls, negative=True, also_bad=(), queries=()):
    """args: the valid argument set (X = a tensor); calls(a, r): the library calls it must make, given the built arguments and the
    method's result; also_bad: further argument sets that must be refused, as overrides of the valid one; queries: the library
    functions the method may ask before it has checked everything"""
    return dict(kind=kind, method=method, args=args, calls=calls, negative=negative, also_bad=also_bad, queries=queries)


def g(a, k):
    return p(a.get(k))


ROWS = [
    # ---- the codec calls ----
    row("SoloBatch", "encode", dict(pcm=X(I16, N, P, L), bits=X(U8, N, P, SLOT, opt=True), nbytes=X(I16, N, P, 2, opt=True), status=X(I32, N, opt=True)),
        lambda a, r: [("solo_batch_encode", H, g(a, "pcm"), P, g(a, "bits"), g(a, "nbytes"), g(a, "status"), None)],
        also_bad=[dict(pcm=X(I16, N, 0, L), bits=X(U8, N, 0, SLOT), nbytes=X(I16, N, 0, 2)), dict(pcm=X(I16, 3, P, L), bits=None, nbytes=None, status=None)]),
    row("SoloBatch", "encode", dict(pcm=X(I16, 3, P, L), streams=LIST),
        lambda a, r: [("solo_batch_encode_streams", H, ANY, 3, g(a, "pcm"), P, p(r[0]), p(r[1]), p(r[2]), None)], negative=False),
    row("SoloBatch", "decode", dict(bits=X(U8, N, P, SLOT), nbytes=X(I16, N, P, 2), recv=X(U8, N, P, opt=True), pcm=X(I16, N, P, L, opt=True),
                                    status=X(I32, N, opt=True)),
        lambda a, r: [("solo_batch_decode", H, g(a, "bits"), g(a, "nbytes"), g(a, "recv"), P, g(a, "pcm"), g(a, "status"), None)],
        also_bad=[dict(bits=X(U8, N, 0, SLOT), nbytes=X(I16, N, 0, 2), recv=None, pcm=None)]),
    row("SoloBatch", "decode", dict(bits=X(U8, 3, P, SLOT), nbytes=X(I16, 3, P, 2), streams=LIST),
        lambda a, r: [("solo_batch_decode_streams", H, ANY, 3, g(a, "bits"), g(a, "nbytes"), None, P, p(r[0]), p(r[1]), None)], negative=False),
    row("SoloBatch", "decode_split", dict(desc_a=X(U8, N, P, 200), len_a=X(I16, N, P), desc_b=X(U8, N, P, 200), len_b=X(I16, N, P),
                                          pcm=X(I16, N, P, L, opt=True), status=X(I32, N, opt=True)),
        lambda a, r: [("solo_batch_decode_split", H, g(a, "desc_a"), g(a, "len_a"), g(a, "desc_b"), g(a, "len_b"), 200, P, g(a, "pcm"), g(a, "status"), None)]),
    row("SoloBatch", "decode_split", dict(desc_a=X(U8, N, P, 200), len_a=X(I16, N, P), desc_b=X(U8, N, P, 200), len_b=X(I16, N, P)),
        lambda a, r: [("solo_batch_decode_split", H, g(a, "desc_a"), g(a, "len_a"), g(a, "desc_b"), g(a, "len_b"), 200, P, p(r[0]), p(r[1]), None)],
        negative=False),
    row("SoloBatch", "recv_insert", dict(arrivals=X(I32, 11, 5, free=(0,)), payload=X(U8, 1000, free=(0,))),
        lambda a, r: [("solo_recv_insert", H, g(a, "arrivals"), 11, g(a, "payload"), 1000, None)]),
    row("SoloBatch", "recv_decode", dict(n_packets=2, pcm=X(I16, N, 2, L, opt=True), status=X(I32, N, opt=True)),
        lambda a, r: [("solo_recv_decode", H, 2, g(a, "pcm"), g(a, "status"), None)],
        also_bad=[dict(n_packets=0, pcm=None), dict(n_packets=-1, pcm=None)]),
    row("SoloBatch", "recv_decode", dict(n_packets=2, streams=LIST),
        lambda a, r: [("solo_recv_decode_streams", H, ANY, 3, 2, p(r[0]), p(r[1]), None)], negative=False),
    # ---- the bridge calls ----
    row("SoloBatch", "recv_report", dict(streams=X(I32, 5, opt=True, seq=True), min_ready=X(I32, 5), max_span=7, clear_margin=True, reports=X(I32, 5, 16, opt=True),
                                         play_list=X(I32, 5, opt=True), play_rows=X(I32, 5, opt=True)),
        lambda a, r: [("solo_recv_report", H, g(a, "streams"), 5, g(a, "min_ready"), 0, 7, 1, g(a, "reports"), g(a, "play_list"), g(a, "play_rows"),
                       p(r[3]), None)]),
    row("SoloBatch", "recv_report", dict(min_ready=2),
        lambda a, r: [("solo_recv_report", H, None, N, None, 2, 0, 0, p(r[0]), p(r[1]), p(r[2]), p(r[3]), None)], negative=False),
    row("SoloBatch", "send_pack", dict(bits=X(U8, N, P, SLOT), nbytes=X(I16, N, P, 2), send=X(U8, N, P, opt=True), first_seq=100, seq_base=X(I32, N, opt=True),
                                       records=X(I32, 10, 5, free=(0,), opt=True), payload=X(U8, 999, free=(0,), opt=True)),
        lambda a, r: [("solo_send_pack", H, g(a, "bits"), g(a, "nbytes"), g(a, "send"), P, g(a, "seq_base"), 100, g(a, "records"), 10, g(a, "payload"), 999,
                       p(r[2]), None)]),
    row("SoloBatch", "send_pack", dict(bits=X(U8, 3, P, SLOT), nbytes=X(I16, 3, P, 2), streams=LIST),
        lambda a, r: [("solo_send_pack_streams", H, ANY, 3, g(a, "bits"), g(a, "nbytes"), None, P, None, 0, p(r[0]), 2 * 3 * P, p(r[1]), 3 * P * SLOT,
                       p(r[2]), None)], negative=False),
    row("SoloBatch", "mix", dict(pcm=X(I16, 5, P, L), room=X(I32, 5), gain=X(I16, 5, opt=True), max_speakers=2, out=X(I16, 5, P, L, opt=True),
                                 energy=X(I64, 5, P, opt=True), mixed=X(U8, 5, P, opt=True)),
        lambda a, r: [("solo_mix", H, g(a, "pcm"), 5, P, g(a, "room"), 5, g(a, "gain"), 2, g(a, "out"), g(a, "energy"), g(a, "mixed"), p(r[1]), None)]),
    row("SoloBatch", "mix", dict(pcm=X(I16, 5, P, L), room=X(I32, 5)),
        lambda a, r: [("solo_mix", H, g(a, "pcm"), 5, P, g(a, "room"), 5, None, 0, p(r[0]), None, None, p(r[1]), None)], negative=False),
    row("SoloBatch", "timescale", dict(pcm=X(I16, 5, 2, L, free=(1,)), out_packets=3, out=X(I16, 5, 3, L, opt=True), shift=X(I32, 5, 24, opt=True),
                                       cost=X(I32, 5, 24, opt=True)),
        lambda a, r: [("solo_timescale", H, g(a, "pcm"), 5, 2, 3, g(a, "out"), g(a, "shift"), g(a, "cost"), p(r[1]), None)]),
    row("SoloBatch", "timescale", dict(pcm=X(I16, 5, 2, L), out_packets=1),
        lambda a, r: [("solo_timescale", H, g(a, "pcm"), 5, 2, 1, p(r[0]), None, None, p(r[1]), None)], negative=False),
    row("SoloBatch", "mix_shared", dict(pcm=X(I16, 5, P, L), room=X(I32, 5), gain=X(I16, 5, opt=True), max_speakers=2, keep=X(U8, 5, opt=True),
                                        slots=X(I32, 5, opt=True), n_rooms=4, energy=X(I64, 5, P, opt=True), mixed=X(U8, 5, P, opt=True),
                                        pcm_spk=X(I16, 5, P, L, opt=True), pcm_room=X(I16, 4, P, L, opt=True)),
        lambda a, r: [("solo_mix_shared", H, g(a, "pcm"), 5, P, g(a, "room"), 4, g(a, "gain"), 2, g(a, "keep"), g(a, "slots"), g(a, "pcm_spk"), p(r[1]), p(r[2]),
                       g(a, "pcm_room"), p(r[4]), p(r[5]), g(a, "energy"), g(a, "mixed"), p(r[6]), None)]),
    row("SoloBatch", "mix_shared", dict(pcm=X(I16, 5, P, L), room=X(I32, 5)),
        lambda a, r: [("solo_mix_shared", H, g(a, "pcm"), 5, P, g(a, "room"), 5, None, 3, None, None, p(r[0]), p(r[1]), p(r[2]), p(r[3]), p(r[4]), p(r[5]),
                       None, None, p(r[6]), None)], negative=False),
    row("SoloBatch", "mix_selected", dict(pcm=X(I16, 5, P, L), room=X(I32, 5), sel=X(U8, 5, P), gain=X(I16, 5, opt=True), keep=X(U8, 5, opt=True),
                                          slots=X(I32, 5, opt=True), n_rooms=4, energy=X(I64, 5, P, opt=True), room_nsel=X(U8, 4, P, opt=True),
                                          pcm_spk=X(I16, 5, P, L, opt=True), pcm_room=X(I16, 4, P, L, opt=True)),
        lambda a, r: [("solo_mix_selected", H, g(a, "pcm"), 5, P, g(a, "room"), 4, g(a, "gain"), g(a, "sel"), g(a, "keep"), g(a, "slots"), g(a, "pcm_spk"),
                       p(r[1]), p(r[2]), g(a, "pcm_room"), p(r[4]), p(r[5]), g(a, "room_nsel"), g(a, "energy"), p(r[6]), None)]),
    row("SoloBatch", "mix_selected", dict(pcm=X(I16, 5, P, L), room=X(I32, 5), sel=X(U8, 5, P)),
        lambda a, r: [("solo_mix_selected", H, g(a, "pcm"), 5, P, g(a, "room"), 5, None, g(a, "sel"), None, None, p(r[0]), p(r[1]), p(r[2]), p(r[3]), p(r[4]),
                       p(r[5]), p(r[7]), None, p(r[6]), None)], negative=False),
    row("SoloBatch", "send_fanout", dict(bits=X(U8, 6, P, SLOT), nbytes=X(I16, 6, P, 2), source=X(I32, 9), dst_stream=X(I32, 9, opt=True),
                                         send=X(U8, 9, P, opt=True), first_seq=100, seq_base=X(I32, 9, opt=True),
                                         records=X(I32, 10, 5, free=(0,), opt=True), payload=X(U8, 999, free=(0,), opt=True)),
        lambda a, r: [("solo_send_fanout", H, g(a, "bits"), g(a, "nbytes"), 6, g(a, "source"), g(a, "dst_stream"), 9, g(a, "send"), P, g(a, "seq_base"), 100,
                       g(a, "records"), 10, g(a, "payload"), 999, p(r[2]), None)]),
    row("SoloBatch", "send_fanout", dict(bits=X(U8, 6, P, SLOT), nbytes=X(I16, 6, P, 2), source=X(I32, 9)),
        lambda a, r: [("solo_send_fanout", H, g(a, "bits"), g(a, "nbytes"), 6, g(a, "source"), None, 9, None, P, None, 0, p(r[0]), 2 * 9 * P, p(r[1]),
                       6 * P * SLOT, p(r[2]), None)], negative=False),
    row("SoloBatch", "export_streams", dict(streams=LIST, which="both", blob=X(U8, 3, 4096, free=(1,), opt=True)),
        lambda a, r: [("solo_batch_state_bytes", H, 3), ("solo_batch_export_streams", H, ANY, 3, 3, g(a, "blob"), 4096, p(r[1]), None)],
        queries=("solo_batch_state_bytes",)),
    row("SoloBatch", "import_streams", dict(streams=LIST, blob=X(U8, 3, 4096, free=(1,)), which="dec"),
        lambda a, r: [("solo_batch_import_streams", H, ANY, 3, 2, g(a, "blob"), 4096, p(r), None)]),
    # ---- the objects beside the handle ----
    row("Resampler", "check", dict(pcm=X(I16, 5, P, 960), rows=X(I32, 5, opt=True), out=X(I16, 5, P, 320, opt=True)), lambda a, r: []),
    row("Resampler", "run", dict(pcm=X(I16, 5, P, 960), rows=X(I32, 5, opt=True, seq=True), out=X(I16, 5, P, 320, opt=True)),
        lambda a, r: [("solo_resample_rows", H, g(a, "rows"), 5, g(a, "pcm"), P, 960, g(a, "out"), p(r[1]), None)]),
    row("Resampler", "run", dict(pcm=X(I16, N, P, 960)), lambda a, r: [("solo_resample", H, g(a, "pcm"), P, 960, p(r), None)], negative=False),
    row("Vad", "run", dict(pcm=X(I16, 5, P, 640, free=(1,)), rows=X(I32, 5, opt=True, seq=True), detail=True, level=True),
        lambda a, r: [("solo_vad", H, g(a, "rows"), 5, g(a, "pcm"), P, 640, p(r["sa"]), p(r["detail"]), p(r["level"]), p(r["count"]), None)]),
    row("Vad", "run", dict(pcm=X(I16, 5, P, 640), level=False),
        lambda a, r: [("solo_vad", H, None, 5, g(a, "pcm"), P, 640, p(r["sa"]), None, None, None, None)], negative=False),
    row("Vad", "select", dict(sa=X(U8, 5, P, 2, free=(2,)), level=X(U8, 5, P), room=X(I32, 5), n_rooms=4, gain=X(I16, 5, opt=True), rows=X(I32, 5, opt=True, seq=True)),
        lambda a, r: [("solo_vad_select", H, g(a, "rows"), 5, g(a, "sa"), g(a, "level"), P, 2, g(a, "room"), 4, (3, 128, 64, 5, 6), g(a, "gain"), p(r["sel"]),
                       p(r["gain_out"]), p(r["keep"]), p(r["dominant"]), p(r["count"]), None)]),
    row("Vad", "get_state", dict(rows=X(I32, 5, free=(0,), opt=True, seq=True)), lambda a, r: [("solo_vad_get_state", H, g(a, "rows"), 5, p(r), None)]),
    row("Vad", "set_state", dict(blob=X(U8, 5, 128), rows=X(I32, 5, opt=True, seq=True)),
        lambda a, r: [("solo_vad_set_state", H, g(a, "rows"), 5, g(a, "blob"), None)]),
]


def _build(args):
    return {k: (v.make() if isinstance(v, X) else v) for k, v in args.items()}


def _row_id(r):
    return "%s.%s(%s)" % (r["kind"], r["method"], ",".join(r["args"]))


def _bad_cases():
    for r in ROWS:
        if r["args"].get("streams") is LIST:     # the list on the device instead: a wrong dtype or rank is refused before it is read
            faults = {"dtype": Dev((3,), I64), "rank": Dev((3, 1), I32)}
            if r["method"] in ("export_streams", "import_streams"):          # (taken as it is there: it must be contiguous too)
                faults["noncontiguous"] = Dev((3,), I32, contiguous=False)
            for fault, value in faults.items():
                yield pytest.param(r, {"streams": value}, id="%s.%s-streams-%s" % (r["kind"], r["method"], fault))
        if not r["negative"]:
            continue
        for name, spec in r["args"].items():
            if isinstance(spec, X):
                for fault, value in spec.faults().items():
                    yield pytest.param(r, {name: value}, id="%s.%s-%s-%s" % (r["kind"], r["method"], name, fault))
        for i, over in enumerate(r["also_bad"]):
            yield pytest.param(r, _build(over), id="%s.%s-also%d" % (r["kind"], r["method"], i))


@pytest.mark.parametrize("r,over", list(_bad_cases()))
def test_bad_argument_raises_before_the_library(r, over):
    kw = dict(_build(r["args"]), **over)
    with pytest.raises(ValueError):
        _call(r, kw, NoLibBut(r["queries"]))


@pytest.mark.parametrize("r", [pytest.param(r, id=_row_id(r)) for r in ROWS])
def test_valid_call_reaches_the_library_as_prototyped(r):
    lib, a = Recorder(), _build(r["args"])
    result = _call(r, a, lib)
    want = r["calls"](a, result)
    assert len(lib.calls) == len(want), lib.calls
    fakes = {v.data_ptr() for v in a.values() if isinstance(v, Dev)}
    for got, exp in zip(lib.calls, want):
        assert len(got) == len(exp), (got, exp)
        for i, (x, y) in enumerate(zip(got, exp)):
            if y is ANY:
                assert isinstance(x, int) and x and x not in fakes, (got[0], i, x)
            else:
                assert type(x) is type(y) and x == y, (got[0], i, x, y)
    if r["method"] == "check":
        assert result == (5, P, 960, 320)


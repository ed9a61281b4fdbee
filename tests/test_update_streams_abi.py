"""Control changes of running streams (solo_batch_update_streams): declared in the header, exported by the built library, bound by
solo_amd, argument errors of the binding; and the oracle of the GPU tests -- mid-stream changes written into the compiled reference's
handle (tests/ref_ctl_poke.py) -- checked against the compiled reference itself.  No compute call on a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import refcodec as R
import solo_amd
import solo_testlib as T

NAME = "solo_batch_update_streams"


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(solo_amd.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return C.CDLL(solo_amd.LIB_PATH)


def test_declared_exported_listed_and_bound(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(T.ROOT, "include", "solo_mi355x.h")).read(), flags=re.S)
    assert re.search(r"\bint32_t\s+%s\s*\(" % NAME, hdr)
    assert hasattr(lib, NAME)
    assert NAME in solo_amd.ABI_SYMBOLS
    loaded = solo_amd.load_library()
    f = getattr(loaded, NAME)
    assert f.restype is C.c_int32 and len(f.argtypes) == 7
    assert callable(getattr(solo_amd.SoloBatch, "update_streams", None))


def test_null_handle_is_refused(lib):
    idx = (C.c_int32 * 1)(0)
    f = getattr(lib, NAME)
    f.restype = C.c_int32
    for which in (1, 2, 3):
        assert f(None, idx, 1, which, None, None, None) == -1


class _NoCall:
    def __getattr__(self, name):
        raise AssertionError("the library was called (%s) although the arguments are wrong" % name)


def _handle(n=4, encoder=True, decoder=True, **kw):
    """a SoloBatch without a device: enough for the argument checks, which run before anything reaches the library"""
    b = object.__new__(solo_amd.SoloBatch)
    b.n_streams, b.lib, b.h = n, _NoCall(), None
    b._enc = solo_amd.default_enc_ctrl(**kw) if encoder else None
    dkw = {k: v for k, v in kw.items() if k in ("joint", "samplerate", "framesize_ms")}
    b._dec = solo_amd.default_dec_ctrl(**dkw) if decoder else None
    return b


@pytest.mark.parametrize("bad", [
    dict(streams=[]), dict(streams=[0, 4]), dict(streams=[-1]), dict(streams=[1, 1]),
    dict(streams=[0, 1], rate=[15600]), dict(streams=[0], dtx=[1, 0]), dict(streams=[0, 1, 2], use_md_index=[1]),
    dict(streams=[0], which="sideways"), dict(streams=[0], rate=24000, which="dec"), dict(streams=[0], dtx=1, which="dec"),
])
def test_binding_argument_errors_raise(bad):
    with pytest.raises(ValueError):
        _handle().update_streams(**bad)


def test_binding_refuses_what_the_handle_lacks():
    with pytest.raises(ValueError):
        _handle(encoder=False).update_streams([0], which="enc")
    with pytest.raises(ValueError):
        _handle(encoder=False).update_streams([0], rate=24000)
    with pytest.raises(ValueError):
        _handle(decoder=False).update_streams([0], which="dec")
    for r in (13600, 14000, 15599):           # the 32 kHz mode: SILK must get >= 14000 bps
        with pytest.raises(ValueError):
            _handle(samplerate=32000, rate=15600).update_streams([1], rate=r)
    with pytest.raises(ValueError):
        _handle(samplerate=32000, rate=15600, joint=1).update_streams([1], rate=14799)


# ---- the oracle: changes written into the compiled reference's handle -------------------------------------------------------------
need_ref = pytest.mark.skipif(not R.have_ref("fix"), reason="oracle/_ref not present on this box")


def _encode(x, sched, **kw):
    import ref_ctl_poke as K
    e = K.PokeEncoder("fix", **kw)
    out = []
    for p in range(x.shape[0]):
        if p in sched:
            e.set_control(**sched[p])
        out.append(e.encode(x[p]))
    return out


@need_ref
@pytest.mark.parametrize("kw", [dict(), dict(rate=24000, dtx=1, use_md_index=1), dict(joint=1), dict(framesize_ms=20)])
def test_poking_the_current_control_changes_nothing(kw):
    import ref_ctl_poke as K
    samples = 640 * kw.get("framesize_ms", 40) // 40
    x = R.synth_stream(77, 16).reshape(-1)[:16 * samples].reshape(16, samples)
    e = K.PokeEncoder("fix", **kw)
    rate, dtx, md = e.control()
    e.close()
    plain = _encode(x, {}, **kw)
    same = {p: dict(rate=rate + (800 if kw.get("joint") else 1600), dtx=dtx, use_md_index=md) for p in (0, 5, 6, 11)}
    assert _encode(x, same, **kw) == plain
    # the decoder: useMDIndex written over with its own value
    pay = plain
    ys = []
    for poke in (False, True):
        d = K.PokeDecoder("fix", use_md_index=kw.get("use_md_index", 0), joint=kw.get("joint", 0), framesize_ms=kw.get("framesize_ms", 40))
        y = []
        for p, (pl, n0, n1) in enumerate(pay):
            if poke and p % 3 == 0:
                d.set_control(use_md_index=kw.get("use_md_index", 0))
            call = (b"", 16, 0, 1) if n0 == 0 else (pl, n0, n1, 4)
            y.append(d.decode(*call)[0])
        ys.append(np.stack(y))
    assert np.array_equal(ys[0], ys[1])


@need_ref
def test_poking_another_rate_moves_later_packets_only():
    x = R.synth_stream(78, 20)
    plain = _encode(x, {})                                         # 13600 bps
    for rate, sign in ((40000, 1), (6000, -1)):
        moved = _encode(x, {8: dict(rate=rate)})
        assert moved[:8] == plain[:8]                              # packets before the change are the same bytes
        assert moved[8:] != plain[8:]
        d = sum(m[1] for m in moved[8:]) - sum(p[1] for p in plain[8:])
        assert d * sign > 0, (rate, d)                             # and later ones grow / shrink with the rate


@need_ref
def test_poking_dtx_and_md_index_takes_effect_at_the_next_packet():
    rng = np.random.default_rng(79)
    x = R.synth_stream(79, 16)
    x[4:14] = (rng.standard_normal((10, 640)) * 3).astype(np.int16)   # a long quiet stretch
    plain = _encode(x, {})
    dtx = _encode(x, {10: dict(dtx=1)})
    assert dtx[:10] == plain[:10] and dtx[10][1] == 0              # DTX switched on late in the silence: the very next packet is dropped
    md = _encode(x, {6: dict(use_md_index=1)})
    assert md[:6] == plain[:6]
    assert md[6:] != plain[6:]                                     # every description now starts with its index

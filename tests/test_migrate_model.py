"""Stream migration (solo_batch_export_streams / solo_batch_import_streams, solo_amd/csrc/solo_migrate.h) without a GPU: the host
forms of the export, the record check and the import are compiled by this test (tests/migrate_host.cpp, through
tests/host_build.py) and run on numpy-made handles -- random bytes as stream records, a small ring with random lengths -- against the
independent numpy model of tests/migrate_model.py: header fields, both checksums, play-relative order of the queue at every wrap
offset, zero fill beyond `len`, every refusal rule, and a refused import that leaves the target as it was."""
import ctypes as C

import numpy as np
import pytest

import migrate_model as M
from host_build import host_lib

ENC_BYTES, DEC_BYTES = 1072, 604          # a multiple of 16 and one that is only a multiple of 4, like the real records


@pytest.fixture(scope="module")
def host():
    lib = host_lib("migrate")
    lib.emu_mig_state_bytes.restype = C.c_longlong
    lib.emu_mig_state_bytes.argtypes = [C.c_void_p, C.c_int]
    common = [C.c_void_p] * 7 + [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p]
    lib.emu_mig_export.argtypes = common
    lib.emu_mig_import.argtypes = common
    lib.emu_mig_sums.argtypes = [C.c_void_p, C.c_longlong, C.c_void_p]
    return lib


def aligned(nbytes, align=16):
    """a zeroed uint8 array whose first byte lies on a 16-byte boundary"""
    raw = np.zeros(nbytes + align, np.uint8)
    off = (-raw.ctypes.data) % align
    return raw[off:off + nbytes]


def make_handle(rng, n_streams, depth=4, slot=48, enc=True, dec=True, ring=True, trk=True, rate=16000, mode=2):
    g = dict(enc_rate=rate if enc else 0, enc_mode=mode if enc else 0, enc_bytes=ENC_BYTES if enc else 0, dec_rate=rate if dec else 0,
             dec_mode=mode if dec else 0, dec_bytes=DEC_BYTES if dec else 0, depth=depth if ring else 0, slot=slot if ring else 0)
    h = dict(g=g, n=n_streams, enc=None, dec=None, ring=None, lens=None, play=None, trk=None)
    if enc:
        h["enc"] = aligned(n_streams * ENC_BYTES).reshape(n_streams, ENC_BYTES)
        h["enc"][:] = rng.integers(0, 256, h["enc"].shape, dtype=np.uint8)
    if dec:
        h["dec"] = aligned(n_streams * DEC_BYTES).reshape(n_streams, DEC_BYTES)
        h["dec"][:] = rng.integers(0, 256, h["dec"].shape, dtype=np.uint8)
    if ring:
        h["ring"] = aligned(n_streams * depth * 2 * slot).reshape(n_streams, depth, 2, slot)
        h["ring"][:] = rng.integers(1, 256, h["ring"].shape, dtype=np.uint8)        # (stale bytes everywhere: none of them is 0)
        la = np.where(rng.random((n_streams, depth)) < 0.3, 0, rng.integers(1, slot + 1, (n_streams, depth)))
        lb = np.where(rng.random((n_streams, depth)) < 0.3, 0, rng.integers(1, slot + 1, (n_streams, depth)))
        la[0, 0], lb[0, 0] = slot, 1                                                 # (a full slot and a single byte)
        h["lens"] = (la | (lb << 16)).astype(np.uint32)
        h["play"] = rng.integers(0, 1000, n_streams).astype(np.int32)
        if trk:
            h["trk"] = rng.integers(0, 2 ** 32, (n_streams, M.TRK_WORDS), dtype=np.uint64).astype(np.uint32)
    return h


def copy_handle(h):
    return {k: (v.copy() if isinstance(v, np.ndarray) else (dict(v) if isinstance(v, dict) else v)) for k, v in h.items()}


def same_handle(a, b):
    return all((a[k] is None and b[k] is None) or np.array_equal(a[k], b[k]) for k in ("enc", "dec", "ring", "lens", "play", "trk"))


def _args(h, streams, which, blob):
    p = lambda x: x.ctypes.data if x is not None else None
    geom = np.array([h["g"][k] for k in M.GEOM], np.int32)
    smap = np.asarray(streams, np.int32)
    cnt = np.zeros(4, np.int32)
    keep = (geom, smap, cnt)
    return [p(h["enc"]), p(h["dec"]), p(h["ring"]), p(h["lens"]), p(h["play"]), p(h["trk"]), p(geom), h["n"], p(smap), len(smap), which, p(blob),
            blob.shape[1], p(cnt)], keep


def count_of(cnt):
    return dict(streams=int(cnt[0]), refused=int(cnt[1]), bytes=int(cnt[2:4].view(np.int64)[0]))


def run_export(host, h, streams, which, stride=None, fill=0xA5):
    stride = stride or M.state_bytes(h["g"], which)
    blob = aligned(len(streams) * stride).reshape(len(streams), stride)
    blob[:] = fill
    args, keep = _args(h, streams, which, blob)
    host.emu_mig_export(*args)
    return blob, count_of(keep[2])


def run_import(host, h, streams, which, blob):
    args, keep = _args(h, streams, which, blob)
    why = host.emu_mig_import(*args)
    return why, count_of(keep[2])


def test_sizes(host):
    import solo_amd
    assert host.emu_mig_count_size() == 16 == C.sizeof(solo_amd.solo_migrate_count_t)
    assert host.emu_mig_geom_size() == 32
    rng = np.random.default_rng(1)
    for depth, slot in ((4, 48), (8, 256), (5, 97), (1, 1)):
        h = make_handle(rng, 1, depth, slot)
        geom = np.array([h["g"][k] for k in M.GEOM], np.int32)
        for which in range(1, 8):
            n = host.emu_mig_state_bytes(geom.ctypes.data, which)
            assert n == M.state_bytes(h["g"], which) and n % 16 == 0, (depth, slot, which)


def test_checksums_wrap(host):
    """both sums against exact integer arithmetic; all-0xFF words make every partial product and both sums wrap"""
    rng = np.random.default_rng(2)
    for nq, kind in ((1, "rand"), (7, "rand"), (1500, "rand"), (1500, "ff"), (70000, "ff")):
        body = aligned(16 * nq)
        body[:] = 0xFF if kind == "ff" else rng.integers(0, 256, 16 * nq, dtype=np.uint8)
        out = np.zeros(2, np.uint32)
        host.emu_mig_sums(body.ctypes.data, nq, out.ctypes.data)
        assert (int(out[0]), int(out[1])) == M.checksums(body), (nq, kind)
    assert M.checksums(np.full(16 * 70000, 0xFF, np.uint8))[0] == (4 * 70000 * 0xFFFFFFFF) % 2 ** 32


@pytest.mark.parametrize("depth,slot", [(4, 48), (4, 41), (8, 256)])
@pytest.mark.parametrize("trk", [True, False])
def test_export_against_model(host, depth, slot, trk):
    """every `which`, a list with gaps, a stride with slack: header fields, sums, body and the untouched slack"""
    rng = np.random.default_rng(10 + depth + slot)
    h = make_handle(rng, 9, depth, slot, trk=trk)
    before = copy_handle(h)
    streams = [1, 4, 6, 8]
    for which in range(1, 8):
        need = M.state_bytes(h["g"], which)
        for stride in (need, need + 32):
            blob, cnt = run_export(host, h, streams, which, stride)
            assert cnt == dict(streams=len(streams), refused=0, bytes=len(streams) * need)
            for i, s in enumerate(streams):
                want = M.export_record(h, s, which)
                assert want.size == need
                hd, whd = blob[i, :64].view(np.uint32), want[:64].view(np.uint32)
                assert hd.tolist() == whd.tolist(), (which, s)
                assert hd[0] == M.MAGIC and hd[1] == M.VERSION and hd[2] == which and hd[3] == s and hd[12] == need - 64 and hd[15] == 0
                assert np.array_equal(blob[i, :need], want), (which, s)
                assert (blob[i, need:] == 0xA5).all()
    assert same_handle(h, before)                                   # export reads only


def test_queue_is_play_relative_at_every_wrap_offset(host):
    """the same queue stored at every rotation of a depth-4 ring gives the same section, and stale bytes beyond `len` never show"""
    rng = np.random.default_rng(20)
    D, slot = 4, 48
    lens = np.array([slot | (5 << 16), 0, 17 << 16, 33 | (48 << 16)], np.uint32)      # by play-relative entry
    pay = rng.integers(1, 256, (D, 2, slot), dtype=np.uint8)
    blobs = []
    for r in range(D):
        for stale in (0x11, 0xEE):
            h = make_handle(rng, 2, D, slot, enc=False, dec=False, trk=False)
            h["ring"][:] = stale
            h["play"][1] = 100 + r                                   # entry of sequence number play: (100 + r) % 4
            for k in range(D):
                e = (100 + r + k) % D
                h["lens"][1, e] = lens[k]
                for d in range(2):
                    n = (int(lens[k]) >> (16 * d)) & 0xFFFF
                    h["ring"][1, e, d, :n] = pay[k, d, :n]
            blob, cnt = run_export(host, h, [1], M.RECV)
            assert cnt["streams"] == 1
            assert np.array_equal(blob[0], M.export_record(h, 1, M.RECV))
            sec = blob[0, 64:].copy()
            assert sec[0:4].view(np.int32)[0] == 100 + r
            sec[0:4] = 0
            blobs.append(sec)
            got = sec[16 + 16:16 + 16 + 2 * D * slot].reshape(D, 2, slot)
            for k in range(D):
                for d in range(2):
                    n = (int(lens[k]) >> (16 * d)) & 0xFFFF
                    assert np.array_equal(got[k, d, :n], pay[k, d, :n]) and (got[k, d, n:] == 0).all(), (r, k, d)
    assert all(np.array_equal(blobs[0], b) for b in blobs[1:])
    # without counters: zeros, margin_min = D
    trk = blobs[0][-48:].view(np.uint32)
    assert trk[M.TRK_MARGIN] == D and trk.sum() == D


@pytest.mark.parametrize("depth,slot", [(4, 48), (4, 41)])
def test_import_against_model(host, depth, slot):
    """records into other slots of another handle, at another wrap offset; a blob with more sections than the call takes; unlisted
    streams untouched; export of the result equals the blob"""
    rng = np.random.default_rng(30 + slot)
    a = make_handle(rng, 9, depth, slot)
    src = [1, 4, 6]
    for blob_which, which in ((7, 7), (7, 2), (7, 5), (3, 1), (6, 4), (4, 4), (1, 1)):
        b = make_handle(rng, 5, depth, slot)
        want = copy_handle(b)
        blob, _ = run_export(host, a, src, blob_which)
        dst = [0, 2, 3]
        why, cnt = run_import(host, b, dst, which, blob)
        assert why == 0 and cnt == dict(streams=3, refused=0, bytes=3 * M.state_bytes(b["g"], which)), (blob_which, which, why, cnt)
        for i, s in enumerate(dst):
            assert M.check_record(blob[i], b["g"], which, blob.shape[1]) == 0
            M.import_record(want, s, blob[i], which)
        # (the ring's bytes beyond `len` are not defined: compare what the model defines, then the whole through a second export)
        for k in ("enc", "dec", "lens", "play", "trk"):
            assert np.array_equal(b[k], want[k]), (blob_which, which, k)
        again, _ = run_export(host, b, dst, which)
        wagain, _ = run_export(host, want, dst, which)
        assert np.array_equal(again, wagain)
        if which == blob_which:
            assert np.array_equal(again[:, 4 * 4:], blob[:, 4 * 4:])        # all but the origin word
            assert again[:, 12:16].view(np.uint32).reshape(-1).tolist() == dst
        for s in (1, 4):                                                      # unlisted
            rest, _ = run_export(host, b, [s], 7)
            orig, _ = run_export(host, want, [s], 7)
            assert np.array_equal(rest, orig)


def test_every_refusal_rule(host):
    rng = np.random.default_rng(40)
    a = make_handle(rng, 6, 4, 48)
    blob, _ = run_export(host, a, [0, 2, 5], 7)
    R = M.REASONS

    def refused(b, which, bl, streams=(1, 2, 3), rec=None):
        before = copy_handle(b)
        why, cnt = run_import(host, b, list(streams), which, bl)
        if why:
            assert same_handle(b, before), "a refused import changed the target"
            assert cnt == dict(streams=-1, refused=rec, bytes=0), (why, cnt)
            if why != R["list"]:
                assert M.check_record(bl[rec - 1], b["g"], which, bl.shape[1]) == why
        return why

    b = make_handle(rng, 4, 4, 48)
    assert refused(b, 7, blob.copy()) == 0                                    # (the untouched blob is accepted)
    b = make_handle(rng, 4, 4, 48)
    # each header word perturbed in turn, in the second record
    expect = {0: "magic", 1: "version", 2: "which", 3: None, 4: "geometry", 5: "geometry", 6: "geometry", 7: "geometry", 8: "geometry", 9: "geometry",
              10: "geometry", 11: "geometry", 12: "length", 13: "checksum", 14: "checksum", 15: "length"}
    for w, name in expect.items():
        bl = blob.copy()
        bl[1, 4 * w:4 * w + 4].view(np.uint32)[0] ^= 0x10 if w != 2 else 0x4      # (which 7 -> 3: the queue is no longer there)
        why = refused(b, 7, bl, rec=2)
        assert why == (R[name] if name else 0), (w, why)
        if name is None:                                                      # (the origin is information only: the import went through)
            b = make_handle(rng, 4, 4, 48)
    # one flipped body bit, in every section and in the padding, in the last record
    for off in (64, 64 + ENC_BYTES + 7, 64 + ENC_BYTES + M.pad16(DEC_BYTES) - 1, blob.shape[1] - 1, blob.shape[1] - 200):
        bl = blob.copy()
        bl[2, off] ^= 0x20
        assert refused(b, 7, bl, rec=3) == R["checksum"], off
        assert refused(b, 1, bl, rec=3) == R["checksum"], off                 # (the sums cover the whole body, whatever the call takes)
    # which not a subset of the blob's sections
    b3, _ = run_export(host, a, [0, 2, 5], 3)
    assert refused(b, 7, np.ascontiguousarray(np.pad(b3, ((0, 0), (0, blob.shape[1] - b3.shape[1])))), rec=1) == R["which"]
    assert refused(b, 4, b3, rec=1) == R["which"]
    # geometry of the handle: rate, mode, record size, ring depth, slot
    for kw, which in ((dict(rate=32000), 1), (dict(rate=32000), 2), (dict(mode=1), 3), (dict(mode=2 | 1 << 16), 2), (dict(depth=8), 4), (dict(slot=64), 4)):
        other = make_handle(rng, 4, **{**dict(depth=4, slot=48), **kw})
        assert refused(other, which, blob, rec=1) == R["geometry"], kw
    other = make_handle(rng, 4, 4, 48)
    other["g"]["dec_bytes"] += 4
    assert refused(other, 2, blob, rec=1) == R["geometry"]
    other = make_handle(rng, 4, depth=8, slot=48)
    assert refused(other, 3, blob) == 0                                       # (the ring differs, the call does not take it)
    # a stride that does not hold the body the header declares
    short = np.ascontiguousarray(blob[:, :blob.shape[1] - 16])
    assert refused(b, 1, short, rec=1) == R["length"]
    # queue words no ring could hold, with sums that are right
    for what in ("play", "len"):
        q = make_handle(rng, 6, 4, 48)
        if what == "play":
            q["play"][2] = -5
        else:
            q["lens"][2, 1] = 49
        bq, _ = run_export(host, q, [0, 2, 5], 4)
        assert refused(b, 4, bq, rec=2) == R["queue"], what
    # the list: not increasing, out of range, negative -- the bad position is the record
    for streams, rec in (((1, 1, 3), 2), ((2, 1, 3), 2), ((0, 1, 4), 3), ((-1, 1, 2), 1)):
        assert refused(b, 7, blob, streams, rec=rec) == R["list"]
    # a refused export list writes streams = -1 and nothing else
    bl, cnt = run_export(host, a, [2, 2, 5], 7)
    assert cnt["streams"] == -1 and (bl == 0xA5).all()

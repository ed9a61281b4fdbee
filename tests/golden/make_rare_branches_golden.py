"""Writes tests/golden/rare_branches.npz from tests/golden/rare_branches_seeds.json (what tools/debug/rare_branch_search.py found: streams
that reach lines of the kernel headers no other input of the suite reaches) and the compiled reference (oracle/_ref).

Per kept stream (at most 32, of 12 packets from a reset): the configuration, the PCM, the receive mask, the reference's payloads and
lengths, CRC-32 of every reference-decoded packet under the mask, the lines the stream is there for.  A stream is kept only if the
-O2 and the -O3 reference agree on it and the host emulation reproduces both (each run in a forked child: the reference has crashes of
its own on extreme inputs).  Data only.

    python tests/golden/make_rare_branches_golden.py
"""
import json
import os
import pickle
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools", "debug")):
    sys.path.insert(0, p)
import refcodec as R  # noqa: E402
import solo_testlib as T  # noqa: E402
import rare_branch_search as S  # noqa: E402

SLOT = 512


def reference(kind, seed, which):
    cfg, pcm, recv = S.stream(kind, seed)
    sr = 32000 if cfg["wb"] else 16000
    e = R.RefEncoder(which, rate=cfg["rate"], joint=cfg["joint"], dtx=0, use_md_index=cfg["mdi"], samplerate=sr)
    d = R.RefDecoder(which, joint=cfg["joint"], use_md_index=cfg["mdi"], samplerate=sr)
    pay, crc = [], []
    for p in range(S.P):
        pl, n0, n1 = e.encode(pcm[p])
        assert 0 < len(pl) == n0 <= SLOT
        m = int(recv[p])
        x, ret = d.decode(pl, n0, n1, 1) if m == 0 else d.decode(*R.map_loss(pl, n0, n1, not (m & 1), not (m & 2)))
        pay.append((pl, n0, n1))
        crc.append((zlib.crc32(x.tobytes()), ret))
    return pay, crc


def forked(fn, *args):
    """fn(*args) in a forked child -> its result, or None if the child died"""
    r, w = os.pipe()
    pid = os.fork()
    if pid == 0:
        os.close(r)
        try:
            os.write(w, pickle.dumps(fn(*args)))
        finally:
            os._exit(0)
    os.close(w)
    data = b""
    while True:
        c = os.read(r, 1 << 16)
        if not c:
            break
        data += c
    os.close(r)
    _, status = os.waitpid(pid, 0)
    return pickle.loads(data) if status == 0 and data else None


def main():
    found = json.load(open(S.SEEDS_FILE))
    assert found["packets"] == S.P
    out, n, dropped = {}, 0, []
    for key, lines in sorted(found["streams"].items())[:32]:
        kind, seed = key.split(":")
        seed = int(seed)
        a, b = forked(reference, kind, seed, "fix"), forked(reference, kind, seed, "fix_O3")
        emu = forked(lambda: [(pay, [(zlib.crc32(x.tobytes()), ret) for x, ret in dec]) for pay, dec in [S.replay(T, R, kind, seed)]][0])
        if a is None or a != b or emu is None or emu[0] != a[0] or emu[1] != a[1] or any(r for _, r in a[1]):
            dropped.append(key)
            continue
        cfg, pcm, recv = S.stream(kind, seed)
        bits, nb = np.zeros((S.P, SLOT), np.uint8), np.zeros((S.P, 2), np.int16)
        for p, (pl, n0, n1) in enumerate(a[0]):
            bits[p, :n0] = np.frombuffer(pl, np.uint8)
            nb[p] = (n0, n1)
        k = "s%02d_" % n
        out[k + "cfg"] = np.array([cfg["wb"], cfg["rate"], cfg["joint"], cfg["mdi"]], np.int32)
        out[k + "pcm"], out[k + "recv"] = pcm, recv
        out[k + "bits"], out[k + "nbytes"] = np.ascontiguousarray(bits[:, :int(nb[:, 0].max())]), nb
        out[k + "dec_crc"] = np.array([c for c, _ in a[1]], np.uint32)
        out[k + "dec_ret"] = np.array([r for _, r in a[1]], np.int32)
        out[k + "what"] = np.array("%s: %s" % (key, ", ".join(lines)))
        n += 1
    out["n_streams"] = np.int32(n)
    out["dropped"] = np.array(", ".join(dropped))
    np.savez_compressed(os.path.join(HERE, "rare_branches.npz"), **out)
    # the outcome goes behind the search's section of the report
    rep, tag = os.path.join(ROOT, "profiles", "emu_coverage.txt"), "rare_branches.npz: "
    lines = [t for t in open(rep).read().split("\n") if not t.startswith(tag)]
    while lines and not lines[-1]:
        lines.pop()
    open(rep, "w").write("\n".join(lines + [tag + "%d of the kept streams confirmed by the compiled reference (-O2 = -O3 = emulation, payloads of at most %d bytes, "
                                            "every packet decoded with status 0); dropped: %s" % (n, SLOT, ", ".join(dropped) or "none"), ""]))
    print("rare_branches.npz: %d streams, dropped (the reference died, decoded with an error, or its two builds or the emulation disagreed): %s" % (n, dropped or "none"))


if __name__ == "__main__":
    main()

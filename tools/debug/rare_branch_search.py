#!/usr/bin/env python3
"""Searches whole-encoder PCM for the lines of the kernel headers that no input of the suite reaches in the host emulation (the lines
tools/debug/emu_coverage.py lists as unreached before the function-level probe; run that tool first: this one uses its coverage build
and its module counters under build/cov).  Host only.

Streams of 12 packets from a reset: the un-speech-like families of solo_amd.synth.edge_stream under the configurations of
tools/debug/fuzz_encoder_emu.py (kinds edge, edge_wb) and speech-like streams at a random level under a random configuration (kind level:
sampling mode, rate, high-band framing, description index); DTX stays off, a dropped packet has no bytes to compare.  Every stream is
encoded by the emulation and decoded under a seeded loss mask.  Workers of 8 streams each run under a GCOV_PREFIX of their own (16 at a
time); when a worker's counters show a wanted line, its streams run again one by one and the first that reaches the line is kept.

The seeds kept go to tests/golden/rare_branches_seeds.json (tests/golden/make_rare_branches_golden.py checks them against the compiled
reference and writes the fixture); the seed ranges searched and the lines still unreached replace the last section of
profiles/emu_coverage.txt.

    python tools/debug/rare_branch_search.py [--minutes 10]
"""
import argparse
import json
import os
import shutil
import sys
import time
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import emu_coverage as E  # noqa: E402

ROOT = E.ROOT
P = 12
CHUNK = 8
KINDS = ("edge", "edge_wb", "level")
CFGS = [dict(rate=13600, joint=0, mdi=0), dict(rate=13600, joint=1, mdi=1), dict(rate=24000, joint=0, mdi=0), dict(rate=10000, joint=0, mdi=0),
        dict(rate=5000, joint=0, mdi=1), dict(rate=40000, joint=1, mdi=0)]
WB_CFGS = [dict(rate=24000, joint=0, mdi=0), dict(rate=24000, joint=1, mdi=0), dict(rate=32000, joint=0, mdi=1), dict(rate=15600, joint=0, mdi=0),
           dict(rate=47000, joint=0, mdi=0)]
SEEDS_FILE = os.path.join(ROOT, "tests", "golden", "rare_branches_seeds.json")
MARK = "== whole-encoder search (tools/debug/rare_branch_search.py)"


def stream(kind, seed):
    """-> (configuration dict: wb, rate, joint, mdi; PCM int16 [P, packet samples]; receive mask uint8 [P], bit 0 / 1 = description 1 / 2 arrived)"""
    import numpy as np
    from solo_amd.synth import EDGE_FAMILIES, edge_stream, synth_stream
    rng = np.random.default_rng(0x5EA2C400 + seed)
    if kind == "edge":
        cfg = dict(CFGS[(seed // EDGE_FAMILIES) % len(CFGS)], wb=0)
        pcm = edge_stream(seed, P)
    elif kind == "edge_wb":
        cfg = dict(WB_CFGS[(seed // EDGE_FAMILIES) % len(WB_CFGS)], wb=1)
        pcm = edge_stream(seed, 2 * P).reshape(P, 1280)
    else:
        wb = int(rng.integers(0, 2))
        cfg = dict(wb=wb, rate=int(rng.integers(15600, 48000)) if wb else int(rng.integers(5000, 40000)), joint=int(rng.integers(0, 2)), mdi=int(rng.integers(0, 2)))
        x = synth_stream(seed, 2 * P if wb else P).astype(np.float64) * float(10.0 ** rng.uniform(-2.0, 0.45))
        pcm = np.clip(np.rint(x), -32768, 32767).astype(np.int16).reshape(P, 1280 if wb else 640)
    recv = rng.integers(0, 4, P).astype(np.uint8)
    recv[0] = 3
    return cfg, np.ascontiguousarray(pcm), recv


def replay(T, R, kind, seed):
    """a stream through the emulation T loads: encode, decode under the mask -> (payloads [(bytes, n0, n1)], decoded PCM per packet)"""
    cfg, pcm, recv = stream(kind, seed)
    flags = cfg["mdi"] | (2 if cfg["joint"] else 0)
    e, d = T.EmuEncoder(cfg["rate"], flags, wb=bool(cfg["wb"])), T.EmuDecoder(flags & 3, wb=bool(cfg["wb"]))
    pay, dec = [], []
    for p in range(P):
        pl, n0, n1 = e.encode(pcm[p])
        pay.append((pl, n0, n1))
        m = int(recv[p])
        dec.append(d.decode(pl, n0, n1, 1) if m == 0 else d.decode(*R.map_loss(pl, n0, n1, not (m & 1), not (m & 2))))
    return pay, dec


def wanted_lines():
    """{(header, line)} that no module of the suite executes (the module workers' counters of tools/debug/emu_coverage.py)"""
    mods = ["module_" + m for m in E.MODULES]
    want = set()
    for h, (L, _) in E.merge(mods).items():
        want |= {(h, ln) for ln, per in L.items() if not any(v > 0 for v in per.values())}
    assert want, "run tools/debug/emu_coverage.py first"
    return want


def lines_hit(name, want):
    got = set()
    for h, (L, _) in E.gcov_counts(name).items():
        got |= {(h, ln) for ln, v in L.items() if v > 0 and (h, ln) in want}
    shutil.rmtree(os.path.join(E.COV, "run", name), ignore_errors=True)
    return got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=10.0)
    a = ap.parse_args()
    want = wanted_lines()
    left, kept, done = set(want), {}, {k: 0 for k in KINDS}
    t_end = time.time() + 60.0 * a.minutes

    def chunk(job):
        kind, s0 = job
        name = "search_%s_%d" % (kind, s0)
        E.run_worker(name, ["streams", kind, str(s0), str(CHUNK)])
        return job, lines_hit(name, want)
    with ThreadPoolExecutor(E.WORKERS) as ex:
        while time.time() < t_end and left and len(kept) < 32:
            jobs = []
            for _ in range(2):
                for k in KINDS:
                    jobs.append((k, done[k]))
                    done[k] += CHUNK
            for (kind, s0), hit in ex.map(chunk, jobs):
                if not hit & left:
                    continue
                for s in range(s0, s0 + CHUNK):          # which stream of the chunk it was
                    name = "search_one_%s_%d" % (kind, s)
                    E.run_worker(name, ["streams", kind, str(s), "1"])
                    new = lines_hit(name, want) & left
                    if new:
                        kept["%s:%d" % (kind, s)] = sorted("%s:%d" % hl for hl in new)
                        left -= new
                        print("%s seed %d reaches %s" % (kind, s, kept["%s:%d" % (kind, s)]), flush=True)
                    if len(kept) >= 32:
                        break
    json.dump({"packets": P, "streams": kept}, open(SEEDS_FILE, "w"), indent=1, sort_keys=True)
    rep = os.path.join(ROOT, "profiles", "emu_coverage.txt")
    txt = open(rep).read()
    txt = txt[:txt.index(MARK)] if MARK in txt else txt.rstrip("\n") + "\n\n"
    reached = want - left
    out = [MARK, "streams of %d packets from a reset, DTX off; seeds searched: %s" % (P, ", ".join("%s 0 .. %d" % (k, done[k] - 1) for k in KINDS)),
           "wanted: the %d lines no module of the suite executes; reached by a stream the search kept (rare_branches_seeds.json): %d" % (len(want), len(reached))]
    for key, v in sorted(kept.items()):
        out.append("  %-16s %s" % (key, ", ".join(v)))
    out.append("still unreached after this search:")
    by = {}
    for h, ln in sorted(want - reached):
        by.setdefault(h, []).append(ln)
    for h, lns in by.items():
        funcs = E.functions_of(h)
        out.append("  %s: %s" % (h, ", ".join("%d (%s)" % (ln, E.function_at(funcs, ln)[0]) for ln in lns)))
    open(rep, "w").write(txt + "\n".join(out) + "\n")
    print("\n".join(out))


if __name__ == "__main__":
    main()

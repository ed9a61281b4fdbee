#!/usr/bin/env python3
"""Which lines and branch outcomes of the kernel headers the suite's inputs reach in the host emulation, and which only the cases of the
function-level probe reach.  Host only (gcov); nothing of it runs on a GPU.

Both emulation libraries are compiled with --coverage into build/cov/ (never into tests/emu).  Then, in forked workers with a GCOV_PREFIX
of their own (at most 16 at a time; one worker = one group of inputs, so every line is attributed to the groups that reach it):
  * "before": each emulation-driven CPU module of tests/ (MODULES below: the fixture files and the seeded families the GPU modules
    replay -- synth_stream, edge_stream, burg_sites_inputs, dot_sites_inputs, the rate-range and long-horizon rows) runs under pytest
    with solo_testlib.load_emu / load_emu_wb answering with the coverage libraries;
  * "after": the same plus every family of tests/golden/fn_cases*.npz through emu_fn (tests/fn_probe_lib.py).
gcov -b turns every worker's counters into per-header line and branch counts; the report lists, per kernel header, every line that
"before" never executes with the function it belongs to, whether that function has a body that only the gfx950 build compiles, and what
reaches it "after" (with the number of executions: a line inside a loop over k candidates runs at most k times per case).

    python tools/debug/emu_coverage.py [--out profiles/emu_coverage.txt] [--skip-modules | --report-only]
"""
import argparse
import glob
import os
import re
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
COV = os.path.join(ROOT, "build", "cov")
HEADERS = ("solo_enc_analysis.h", "solo_common.h", "solo_enc_front.h", "solo_enc.h", "solo_dec.h", "solo_rc.h")
MODULES = ("test_emu_encoder", "test_emu_decoder", "test_enc_stages", "test_dec_stages", "test_dec_constructed", "test_pinned_corners", "test_wb",
           "test_nsq_taps", "test_framesize20", "test_long_horizon", "test_pulse_coder", "test_recv_ring", "test_burg_sites_reference",
           "test_dot_sites_reference")
WORKERS = 16
SEARCH_MARK = "== whole-encoder search (tools/debug/rare_branch_search.py)"

# run inside a worker: pytest on one module, or one family of the probe's cases, with the coverage libraries in place of tests/emu's
BOOT = r"""
import ctypes, os, sys
root, cov, what = sys.argv[1], sys.argv[2], sys.argv[3:]
for p in (root, os.path.join(root, "oracle"), os.path.join(root, "tests")):
    sys.path.insert(0, p)
import solo_testlib as T
def _load(wb):
    def load():
        key = "_cov_wb" if wb else "_cov"
        if not hasattr(T, key):
            lib = ctypes.CDLL(os.path.join(cov, "wb" if wb else "nb", "libsolo_emu.so"))
            lib.emu_dec_create.restype = ctypes.c_void_p
            lib.emu_dec_create.argtypes = [ctypes.c_int]
            lib.emu_dec_destroy.argtypes = [ctypes.c_void_p]
            lib.emu_dec_packet.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
            lib.emu_enc_create.restype = ctypes.c_void_p
            lib.emu_enc_create.argtypes = [ctypes.c_int, ctypes.c_int]
            lib.emu_enc_destroy.argtypes = [ctypes.c_void_p]
            lib.emu_enc_packet.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
            setattr(T, key, lib)
        return getattr(T, key)
    return load
T.load_emu, T.load_emu_wb = _load(False), _load(True)
if what[0] == "module":
    import pytest
    sys.exit(pytest.main(["-q", "-x", "-p", "no:cacheprovider", os.path.join(root, "tests", what[1] + ".py"), "-m", "not gpu"]))
if what[0] == "streams":         # tools/debug/rare_branch_search.py: whole-encoder streams
    sys.path.insert(0, os.path.join(root, "tools", "debug"))
    import refcodec as R
    import rare_branch_search as S
    for seed in range(int(what[2]), int(what[2]) + int(what[3])):
        S.replay(T, R, what[1], seed)
    sys.exit(0)
import fn_probe_lib as F
build = F.Build(what[1] == "wb")
recs, _ = F.load_cases(build, what[2])[what[3]]
for site in build.groups[what[2]][1]:
    F.run_emu(build, what[2], recs, site)
"""


def build_cov():
    src = os.path.join(ROOT, "tests", "emu", "solo_emu.cpp")
    for name, flags in (("nb", []), ("wb", ["-DSX_FS_KHZ=16"])):
        d = os.path.join(COV, name)
        os.makedirs(d, exist_ok=True)
        obj = os.path.join(d, "solo_emu.o")
        subprocess.check_call(["g++", "--coverage", "-O2", "-g", "-std=c++17", "-fPIC", "-fwrapv", "-fno-strict-aliasing", "-w", "-DSOLO_HOST_EMU"] + flags +
                              ["-c", src, "-o", obj])
        subprocess.check_call(["g++", "--coverage", "-shared", obj, "-o", os.path.join(d, "libsolo_emu.so")])


def run_worker(name, args):
    """one group of inputs under its own GCOV_PREFIX -> (name, exit status)"""
    prefix = os.path.join(COV, "run", name)
    shutil.rmtree(prefix, ignore_errors=True)
    os.makedirs(prefix)
    env = dict(os.environ, GCOV_PREFIX=prefix, OMP_NUM_THREADS="1")
    with open(os.path.join(prefix, "log.txt"), "w") as log:
        r = subprocess.call([sys.executable, "-c", BOOT, ROOT, COV] + args, env=env, stdout=log, stderr=subprocess.STDOUT, cwd=ROOT)
    return name, r


LINE = re.compile(r"^\s*([^:]+):\s*(\d+):")


def gcov_counts(name):
    """a worker's counters through gcov -b -> {header: ({line: executions}, {line: [taken counts of its branch outcomes]})}"""
    prefix = os.path.join(COV, "run", name)
    got = {}
    for b in ("nb", "wb"):
        gcda = glob.glob(os.path.join(prefix, "**", b, "solo_emu.gcda"), recursive=True)
        if not gcda:
            continue
        work = os.path.join(prefix, "gcov_" + b)
        os.makedirs(work, exist_ok=True)
        shutil.copy(gcda[0], os.path.join(work, "solo_emu.gcda"))
        shutil.copy(os.path.join(COV, b, "solo_emu.gcno"), os.path.join(work, "solo_emu.gcno"))
        subprocess.check_call(["gcov", "-b", "-o", work, os.path.join(ROOT, "tests", "emu", "solo_emu.cpp")], cwd=work, stdout=subprocess.DEVNULL,
                              stderr=subprocess.DEVNULL)
        for h in HEADERS:
            f = os.path.join(work, h + ".gcov")
            if not os.path.exists(f):
                continue
            lines, branches = got.setdefault(h, ({}, {}))
            cur = None
            for t in open(f, errors="replace"):       # (the per-instantiation sections of templates repeat their lines with partial counts: the maximum is the total)
                m = LINE.match(t)
                if m:
                    c, ln = m.group(1).strip(), int(m.group(2))
                    cur = ln
                    if c == "-" or ln == 0:
                        continue
                    v = 0 if c.startswith(("#", "=")) else int(c.rstrip("*"))
                    lines[ln] = max(lines.get(ln, 0), v)
                elif t.startswith("branch") and cur is not None:
                    mm = re.match(r"branch\s+(\d+)\s+(never executed|taken (\d+))", t)
                    if mm:
                        lst = branches.setdefault(cur, {})
                        i = int(mm.group(1))
                        lst[i] = max(lst.get(i, 0), int(mm.group(3) or 0))
    return got


def functions_of(header):
    """[(first line, name, has a body that only the gfx950 build compiles)] of a kernel header, by a plain scan of its text"""
    txt = open(os.path.join(ROOT, "solo_amd", "csrc", header)).read().split("\n")
    starts = []
    pat = re.compile(r"^(?:template\s*<[^>]*>\s*)?(?:SX_FN1|SX_FNW|SX_FN|SX_HD|SX_ENTER_FN|static|inline|constexpr)\b[^;=(]*?\b(\w+)\s*\(")
    for i, t in enumerate(txt):
        m = pat.match(t)
        if m:
            starts.append((i + 1, m.group(1)))
    out = []
    for k, (ln, name) in enumerate(starts):
        end = starts[k + 1][0] - 1 if k + 1 < len(starts) else len(txt)
        body = "\n".join(txt[ln - 1:end])
        out.append((ln, name, "__HIP_DEVICE_COMPILE__" in body or "SX_LANE_STREAM" in body))
    return out


def function_at(funcs, line):
    best = ("?", False)
    for ln, name, dev in funcs:
        if ln <= line:
            best = (name, dev)
    return best


def merge(names):
    """-> {header: ({line: {worker: executions}}, {line: {outcome: {worker: taken}}})}"""
    tot = {}
    for n in names:
        for h, (lines, branches) in gcov_counts(n).items():
            L, B = tot.setdefault(h, ({}, {}))
            for ln, v in lines.items():
                L.setdefault(ln, {})[n] = v
            for ln, d in branches.items():
                for i, v in d.items():
                    B.setdefault(ln, {}).setdefault(i, {})[n] = v
    return tot


NAMED = {"solo_enc_analysis.h": (50, 111, 138, 1011, 1012, 1314, 1315, 1365, 1366, 1643, 1834, 1838, 1866, 1879, 1889, 1923, 1924, 1984, 1985),
         "solo_common.h": (203, 226, 237, 242, 329, 330, 357, 358), "solo_enc_front.h": (509,), "solo_rc.h": (156, 159, 398, 401)}


def notes(F):
    """what gcov on the host build cannot say: the arms that exist as gfx950-only code, and the cases of the fixtures that reach them (the
    conditions tests/test_fn_probe_reference.py asserts), counted from the fixtures"""
    import numpy as np
    out = ["== arms of the gfx950-only bodies (no host line): cases of tests/golden/fn_cases*.npz that reach them, run on the GPU by tests/test_gpu_fn_probe.py"]
    for b in ("nb", "wb"):
        build = F.Build(b == "wb")
        z = np.load(build.fixture)
        for g, (unit, sites, d) in build.groups.items():
            cases = F.load_cases(build, g)
            n = {}
            for fam, (recs, res) in cases.items():
                for i in range(len(recs)):
                    if unit == F.A2NLSF:
                        for c in F.a2nlsf_class(recs[i], res[i], d)[1]:
                            n[c] = n.get(c, 0) + 1
                    elif unit == F.NLSF2A:
                        k = "row form declined (fall-back to the serial form)" if int(res[i, 16]) else "row form accepted"
                        n[k] = n.get(k, 0) + 1
                    elif unit == F.MSVQ:
                        for k, hit in (("exact tie among the best 17 of stage 0", F.msvq_stage0_tie(build, recs[i])), ("survivors cut to 8 in stage 0", F.msvq_stage0_cut(build, recs[i]))):
                            n[k] = n.get(k, 0) + bool(hit)
                    elif unit == F.FIND_LPC:
                        k = "interpIndex %d" % int(res[i, 16])
                        n[k] = n.get(k, 0) + 1
                if unit == F.A2NLSF:
                    n["|ylo| >= 65536 in the pass that succeeds"] = n.get("|ylo| >= 65536 in the pass that succeeds", 0) + int(z["%s/%s/big_ylo" % (g, fam)].sum())
                if unit == F.BURG:
                    sl, nb, D = build.burg_shape(sites[0])
                    n["|num| >= den exit"] = n.get("|num| >= den exit", 0) + int(F.burg_exits(build, sites[0], recs).sum())
                    n["rshifts > MAX_RSHIFTS"] = n.get("rshifts > MAX_RSHIFTS", 0) + sum(F.burg_rshifts(r[:sl * nb]) > 7 for r in recs)
            out.append("%s %-18s sites %-7s %5d cases: %s" % (b, g, ",".join(str(s) for s in sites), sum(len(r) for r, _ in cases.values()),
                                                               "; ".join("%s = %d" % kv for kv in sorted(n.items()))))
    pools = {}
    for b in ("nb", "wb"):
        build = F.Build(b == "wb")
        z = np.load(build.fixture)
        for g in build.groups:
            pools[b, g] = (sum(int(z["%s/%s/dropped" % (g, fam)][2]) for fam in F.GROUP_FAMILIES[g]), sum(len(r) for r, _ in F.load_cases(build, g).values()))
    out += ["", "Not reached by any family, with the search spent (pool = records the families generate, of which the fixture keeps a selection):",
            "  solo_common.h:203 (NLSF2A still beyond int16 after ten limiter rounds): 0 of %s non-decreasing NLSF vectors (pools of nlsf2a_stable / _hb, 16 kHz and 32 kHz builds);"
            % " / ".join(str(pools[b, g][0]) for b in ("nb", "wb") for g in ("nlsf2a_stable", "nlsf2a_stable_hb")),
            "  the |num| >= den exit at the second-half site of the 16 kHz build (2 x 50 samples): 0 of the %d records of burg_1 above (full-scale alternations, DC,"
            % pools["nb", "burg_1"][1],
            "    square waves of every period, periodic blocks and impulses at every level); the 32 kHz build reaches it at that site;",
            "  solo_enc_analysis.h:1923-1924 (the second-half run of Burg scaled further down than the whole-frame run): 0 of %d find_lpc records per build,"
            % pools["nb", "find_lpc"][1],
            "    asserted to stay 0 by tests/test_fn_probe_reference.py: the whole frame's energy contains the second half's, so its shift is never the smaller one;",
            "  solo_enc_analysis.h:1365-1366: the correlation without packed pairs needs a subframe that does not start on a 4-byte boundary, which",
            "    no call site has;",
            "  solo_common.h:237, 242 (sx_nlsf2a_stable): the same two statements as :221 and :226 of sx_nlsf2a_stable_ws, the form with caller-provided work",
            "    space that the encoder, the decoder's parameter path and the probe's fall-back use (its arms are reached, see :226 above).  The form without",
            "    work space is called by the decoder's comfort-noise generator alone (solo_dec.h:1072, 1088) on smoothed NLSF vectors; no function-level case",
            "    goes through it, and no decoder input of the suite makes its filter unstable: still unreached;",
            "  sx_limit_warped_coefs' iteration, sx_schur64's reset, solo_enc_analysis.h:1011-1012, solo_common.h:329-330, solo_enc_front.h:509 and the two-byte",
            "    renormalisation of both range coders (solo_rc.h:156-159, 398-401) have no exported reference function: only whole-encoder PCM can reach",
            "    them; what the search for such PCM spent is in the last section.", ""]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "emu_coverage.txt"))
    ap.add_argument("--skip-modules", action="store_true", help="reuse the module workers' counters of an earlier run")
    ap.add_argument("--report-only", action="store_true", help="reuse every worker's counters of an earlier run")
    a = ap.parse_args()
    for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import fn_probe_lib as F
    a.skip_modules |= a.report_only
    if not a.skip_modules:          # (a rebuild stamps new .gcno files: the counters of an earlier run would no longer belong to them)
        build_cov()
    jobs = [] if a.skip_modules else [("module_" + m, ["module", m]) for m in MODULES]
    fams = []
    for b in ("nb", "wb"):
        build = F.Build(b == "wb")
        for g in build.groups:
            for fam in F.GROUP_FAMILIES[g]:
                fams.append("fn_%s_%s_%s" % (b, g, fam))
                if not a.report_only:
                    jobs.append((fams[-1], ["fn", b, g, fam]))
    with ThreadPoolExecutor(WORKERS) as ex:
        for name, r in ex.map(lambda j: run_worker(*j), jobs):
            print("%-60s %s" % (name, "ok" if r == 0 else "exit %d (see build/cov/run/%s/log.txt)" % (r, name)), flush=True)
    mods = ["module_" + m for m in MODULES]
    tot = merge(mods + fams)
    # every worker of the probe's cases must have left counters; a module that loads the emulation by a path of its own leaves none
    blind = [n for n in mods + fams if not glob.glob(os.path.join(COV, "run", n, "**", "solo_emu.gcda"), recursive=True)]
    assert not set(blind) & set(fams) and len(blind) <= 3, blind
    out = ["Host-emulation coverage of the kernel headers (tools/debug/emu_coverage.py; gcov -b on tests/emu built with --coverage, -O2).",
           "before = the emulation-driven CPU modules of tests/ (%s)," % ", ".join(MODULES),
           "(no counters, the module loads the emulation itself: %s)" % (", ".join(n[7:] for n in blind) or "none"),
           "after  = the same plus the cases of the function-level probe (tests/golden/fn_cases*.npz through emu_fn).",
           "Listed: every line with code that `before` never executes.  dev = the function has a body that only the gfx950 build compiles",
           "(the probe's GPU test, tests/test_gpu_fn_probe.py, runs that body on the cases that reach the line here).", ""]
    for h in HEADERS:
        if h not in tot:
            continue
        L, B = tot[h]
        funcs = functions_of(h)

        def share(ws):
            tk = al = 0
            for ln, d in B.items():
                for i, per in d.items():
                    al += 1
                    tk += any(v > 0 for n, v in per.items() if n in ws)
            return tk, al
        tb, ab = share(set(mods))
        ta, aa = share(set(mods + fams))
        out.append("== %s: branch outcomes taken at least once: before %d of %d (%.1f %%), after %d of %d (%.1f %%)" % (
            h, tb, ab, 100.0 * tb / max(ab, 1), ta, aa, 100.0 * ta / max(aa, 1)))
        out.append("%11s  %-34s %-3s  %-10s  %s" % ("lines", "function", "dev", "before", "after"))
        rows = []                   # (first line, last line, function, dev, after): neighbouring lines with the same answer share a row
        for ln in sorted(L):
            per = L[ln]
            if any(v > 0 for n, v in per.items() if n in mods):
                continue
            name, dev = function_at(funcs, ln)
            reach = sorted(((v, n) for n, v in per.items() if v > 0 and n in fams), reverse=True)
            after = "still unreached" if not reach else "fn_cases: %d executions, %s" % (
                sum(v for v, _ in reach), ", ".join("%s (%d)" % (n[3:], v) for v, n in reach[:3]) + (" ..." if len(reach) > 3 else ""))
            key = sorted(n for _, n in reach)          # (the counts shown are those of the row's first line)
            if rows and rows[-1][2:4] == (name, dev) and rows[-1][5] == key and ln - rows[-1][1] <= 3:
                rows[-1] = (rows[-1][0], ln) + rows[-1][2:]
            else:
                rows.append((ln, ln, name, dev, after, key))
        for a0, a1, name, dev, after, _ in rows:
            out.append("%11s  %-34s %-3s  %-10s  %s" % (str(a0) if a0 == a1 else "%d-%d" % (a0, a1), name, "yes" if dev else "no", "unreached", after))
        # branch outcomes never taken by `before`, per function: line (outcomes never taken / outcomes of the line), * = taken by the probe's cases
        never = {}
        for ln in sorted(B):
            miss = [i for i, per in B[ln].items() if not any(v > 0 for n, v in per.items() if n in mods)]
            if miss:
                got = sum(any(v > 0 for n, v in B[ln][i].items() if n in fams) for i in miss)
                never.setdefault(function_at(funcs, ln), []).append("%d (%d/%d%s)" % (ln, len(miss), len(B[ln]), ", %d*" % got if got else ""))
        out.append("branch outcomes `before` never takes: function [dev]: line (never taken / outcomes of the line, n* = n of them taken by fn_cases)")
        for (name, dev), v in never.items():
            out.append("  %s%s: %s" % (name, " [dev]" if dev else "", ", ".join(v)))
        out.append("")
    # the lines whose absence from every fixture started this report, one by one (a line the optimiser folds into a neighbour has no
    # counter of its own: it is listed with the next line that has one)
    out += ("== the lines that no input of the suite had reached when the probe was written (host emulation of the 16 kHz / 32 kHz builds;",
               "   at -O2 a statement may share its counter with the test in front of it, so the table above is the stricter statement)")
    for h, lns in NAMED.items():
        L = tot.get(h, ({}, {}))[0]
        funcs = functions_of(h)
        for ln in lns:
            at = next((k for k in range(ln, ln + 6) if k in L), None)
            if at is None:
                out.append("%-20s %5d  %-28s no counter (no code of its own in this build)" % (h, ln, function_at(funcs, ln)[0]))
                continue
            per = L[at]
            m = sorted(n[7:] for n, v in per.items() if v > 0 and n in mods)
            f = sorted(((v, n[3:]) for n, v in per.items() if v > 0 and n in fams), reverse=True)
            what = []
            if m:
                what.append("reached by the suite's inputs (%s)" % ", ".join(m[:3]))
            if f:
                what.append("reached by fn_cases (%d families; %s)" % (len(f), ", ".join("%s: %d" % (n, v) for v, n in f[:3])))
            out.append("%-20s %5d%s %-28s %s" % (h, ln, "" if at == ln else " (counted at %d)" % at, function_at(funcs, ln)[0],
                                                "; ".join(what) or "still unreached"))
    out.append("")
    out += notes(F)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    search = ""                     # (the section tools/debug/rare_branch_search.py adds stays)
    if os.path.exists(a.out) and SEARCH_MARK in open(a.out).read():
        old = open(a.out).read()
        search = old[old.index(SEARCH_MARK):]
    open(a.out, "w").write("\n".join(out) + "\n" + search)
    print("wrote", a.out)


if __name__ == "__main__":
    main()

"""Writes tests/golden/fn_cases.npz and fn_cases_wb.npz: the cases of the function-level probe (tests/fn_probe_lib.py) with the compiled
reference's outputs.  Needs oracle/_ref (libsolo_ref_fix.so and libsolo_ref_fix_O3.so).

Per group and family: the family's pool goes through the -O2 and the -O3 reference in forked children; records on which either dies or
on which the two disagree are dropped (counted in <group>/<family>/dropped = [died, disagreed, pool size]); of the rest a selection is
kept -- by class, so that every branch the family is there for keeps its cases -- as indices into the pool (<...>/sel) or, for the families
of fn_probe_lib.STORED, as the records themselves (<...>/in); <...>/out = the reference's output records, <...>/crc = crc32 of the records.

    python tests/golden/make_fn_cases.py [nb|wb]
"""
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import fn_probe_lib as F  # noqa: E402


def pick(classes, names, per_class):
    """indices: up to per_class cases of every class, in pool order"""
    keep = set()
    for c in names:
        keep.update([i for i, cs in enumerate(classes) if c in cs][:per_class])
    return sorted(keep)


def select(build, group, fam, recs, out):
    """-> (indices kept, {class: cases of it among the kept})"""
    unit, sites, d = build.groups[group]
    n, labels = len(recs), {}
    if unit == F.A2NLSF:
        classes = []
        for i in range(n):
            r, cs = F.a2nlsf_class(recs[i], out[i], d)
            # the whole function restated: checks the restatement against the reference, finds the |ylo| >= 65536 arm
            nl, a_left, retries, big_failed, big = F.a2nlsf_full(recs[i], d)
            assert nl == [int(v) for v in out[i, :d]] and a_left == [int(v) for v in out[i, 16:16 + d]], (group, fam, i)
            assert r in (retries, -1) or nl == F.a2nlsf_fallback(d), (group, fam, i, r, retries)
            if big:
                cs.add(F.A2NLSF_BIG)
            if big_failed:
                cs.add("big_ylo_failed_pass")
            classes.append(cs)
        names = F.A2NLSF_CLASSES + (F.A2NLSF_BIG, "big_ylo_failed_pass")
        keep = pick(classes, names, 40)
        labels["big_ylo"] = np.array([F.A2NLSF_BIG in classes[i] for i in keep], np.uint8)
    elif unit == F.NLSF2A:
        ref = F.Ref()
        classes = []
        for i in range(n):
            a32 = F.nlsf2a_a32([int(v) for v in recs[i, :d]], d)
            lim = F.nlsf2a_limit(a32)[0]
            plain = ref.nlsf2a(recs[i], d)
            assert [int(v) for v in plain] == lim, (group, fam, i)                   # the restatement of SKP_Silk_NLSF2A
            classes.append(F.nlsf2a_class(recs[i], d, ref.unstable(plain, d), out[i]))
        names = F.NLSF2A_CLASSES
        keep = pick(classes, names, 48)
    elif unit == F.MSVQ:
        classes = []
        for i in range(n):
            cs = {"sig%d_deact%d" % (int(recs[i, 48]), int(recs[i, 51]))}
            if F.msvq_stage0_tie(build, recs[i]):
                cs.add("tie")
            if F.msvq_stage0_cut(build, recs[i]):
                cs.add("cut")
            classes.append(cs)
        names = ("tie", "cut", "sig0_deact0", "sig0_deact1", "sig1_deact0", "sig1_deact1")
        keep = pick(classes, names, 120 if fam == "midpoints" else 60)
        if fam == "midpoints":
            keep = [i for i in keep if "tie" in classes[i]]
        ref = F.Ref()
        for i in keep:      # the weights are the reference's SKP_Silk_NLSF_VQ_weights_laroia of the target
            assert [int(v) for v in recs[i, 32:32 + d]] == [int(v) for v in ref.weights(recs[i], d)], (group, fam, i)
    elif unit == F.BURG:
        sl, nb, D = build.burg_shape(sites[0])
        ex = F.burg_exits(build, sites[0], recs)
        classes = [({"exit"} if ex[i] else set()) | ({"rshifts_above_7"} if F.burg_rshifts(recs[i, :sl * nb]) > 7 else set()) for i in range(n)]
        for i in range(n):
            assert not ex[i] or F.burg_exit_order(out[i, 2:], D) > 0, (group, fam, i)
        names, keep = ("exit", "rshifts_above_7"), list(range(n))
    else:
        classes, names, keep = [set() for _ in range(n)], ("interp0", "interp1", "interp2", "interp3", "interp4"), list(range(n))
        for i in range(n):
            classes[i].add("interp%d" % int(out[i, 16]))
    counts = {c: sum(1 for i in keep if c in classes[i]) for c in names}
    return keep, counts, labels


def make(wb):
    build = F.Build(wb)
    data, report = {}, []
    ref = F.Ref()
    for group in build.groups:
        unit = build.groups[group][0]
        for fam in F.GROUP_FAMILIES[group]:
            recs = F.pool(build, group, fam, ref)
            o2, ok2 = F.run_ref(build, group, recs, "fix")
            o3, ok3 = F.run_ref(build, group, recs, "fix_O3")
            died = ~(ok2 & ok3)
            differ = ~died & (o2 != o3).any(axis=1)
            good = np.nonzero(~died & ~differ)[0]
            assert int(differ.sum()) * 100 <= len(recs), (group, fam, int(differ.sum()))
            keep, counts, labels = select(build, group, fam, recs[good], o2[good])
            idx = good[keep]
            for name, v in labels.items():
                data["%s/%s/%s" % (group, fam, name)] = v
            emu = F.run_emu(build, group, recs[idx])
            ow = 16 if unit == F.NLSF2A else emu.shape[1]
            bad = int((emu[:, :ow] != o2[idx][:, :ow]).any(axis=1).sum())
            k = "%s/%s" % (group, fam)
            if (group, fam) in F.STORED:
                data[k + "/in"] = recs[idx]
            else:
                data[k + "/sel"] = idx.astype(np.int32)
            data[k + "/out"] = o2[idx]
            data[k + "/crc"] = np.uint32(zlib.crc32(np.ascontiguousarray(recs[idx]).tobytes()))
            data[k + "/dropped"] = np.array([int(died.sum()), int(differ.sum()), len(recs)], np.int32)
            line = "%-18s %-24s pool %5d died %4d O2!=O3 %3d kept %4d emu!=ref %3d  %s" % (group, fam, len(recs), died.sum(), differ.sum(), len(idx), bad,
                                                                                           " ".join("%s=%d" % kv for kv in counts.items()))
            print(line, flush=True)
            report.append(line)
    np.savez_compressed(build.fixture, **data)
    print("%s: %d bytes" % (build.fixture, os.path.getsize(build.fixture)))
    return report


if __name__ == "__main__":
    which = sys.argv[1:] or ["nb", "wb"]
    for w in which:
        make(w == "wb")

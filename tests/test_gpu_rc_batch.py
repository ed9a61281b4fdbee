"""The range coder batched over chunks (SOLO_ENC_RC_BATCH = k packets per coder launch, solo_enc_rc_batch_kernel) is a schedule, not an
algorithm: payload bytes, byte counts and status equal those of the same library with one coder launch per chunk (k = 1), bytes no
kernel may touch included, and those of the compiled reference.  The knob is read when a handle sets its pipeline up, so each value runs
in a child process of its own (tests/rc_batch_worker.py: the cases), once for the whole module."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import rc_batch_worker as W
import refcodec as R

pytestmark = pytest.mark.gpu

KS = (2, 5)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """knob value -> the arrays its child process left: k = 1 over the cases of both batch sizes, k = 2 and k = 5 over their own"""
    d = tmp_path_factory.mktemp("rc_batch")
    out = {}
    for knob, ks in ((1, KS), (2, (2,)), (5, (5,))):
        path = str(d / ("k%d.npz" % knob))
        env = dict(os.environ)
        env.pop("SOLO_ENC_GROUP", None)
        r = subprocess.run([sys.executable, os.path.join(W.ROOT, "tests", "rc_batch_worker.py"), str(knob), ",".join(str(k) for k in ks), path],
                           env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        out[knob] = dict(np.load(path))
    return out


@functools.lru_cache(maxsize=None)
def _ref_stream(kind, ctor, n, row, total):
    """the compiled reference over one stream of a case's input: [(payload, n0, n1)] per packet"""
    pcm = _pcm(kind, n, total)[row]
    e = R.RefEncoder("fix", **dict(ctor))
    return [e.encode(pcm[p]) for p in range(total)]


@functools.lru_cache(maxsize=None)
def _pcm(kind, n, total):
    return W.pcm_of(kind, n, total)


def _check(runs, k, name):
    case = W.cases(k)[name]
    slot = case.get("slot", 512)
    some_fit = some_not = some_dtx = False
    for i, (p0, n) in enumerate(case["calls"]):
        key = "%s/%d/" % (name, i)
        bits, nb, st = (runs[k][key + f] for f in ("bits", "nb", "st"))
        bits1, nb1, st1 = (runs[1][key + f] for f in ("bits", "nb", "st"))
        rows = W.rows_of(case, i)
        assert bits.shape == (len(rows), n, slot)
        # one coder launch per chunk: every byte of every slot, written or not
        assert np.array_equal(st, st1), (name, i, np.nonzero(st != st1)[0][:8])
        assert np.array_equal(nb, nb1), (name, i, np.argwhere(nb != nb1)[:8])
        assert np.array_equal(bits, bits1), (name, i, np.argwhere(bits != bits1)[:8])
        some_not |= bool((st != 0).any())
        some_fit |= bool((nb[:, :, 0] > 0).any())
        if not R.have_ref("fix"):
            continue
        # the compiled reference
        ctor = tuple(sorted(case["ctor"].items()))
        for r, s in enumerate(rows):
            ref = _ref_stream(case["kind"], ctor, case["n"], s, case["total"])
            first_err = 0
            for p in range(n):
                pl, n0, n1 = ref[p0 + p]
                if case["ctor"].get("dtx") and n0 == 0:          # a DTX packet: no low-band bytes, the high band's in the slot
                    some_dtx = True
                    assert (int(nb[r, p, 0]), int(nb[r, p, 1])) == (0, 0), (name, i, s, p)
                    hb = len(pl)
                    assert bits[r, p, :hb].tobytes() == pl and (bits[r, p, hb:] == W.FILL).all(), (name, i, s, p)
                elif n0 > slot:                                  # does not fit: lengths zeroed, slot untouched, first error of the call
                    first_err = first_err or -1
                    assert (int(nb[r, p, 0]), int(nb[r, p, 1])) == (0, 0), (name, i, s, p)
                    assert (bits[r, p] == W.FILL).all(), (name, i, s, p)
                else:
                    assert (int(nb[r, p, 0]), int(nb[r, p, 1])) == (n0, n1), (name, i, s, p)
                    assert bits[r, p, :n0].tobytes() == pl[:n0] and (bits[r, p, n0:] == W.FILL).all(), (name, i, s, p)
            assert int(st[r]) == first_err, (name, i, s)
    return some_fit, some_not, some_dtx


@pytest.mark.parametrize("k,n,p", [(k, n, p) for k in KS for n in W.STREAMS for p in W.packets_of(k)])
def test_plain_streams(runs, k, n, p):
    """streams in {1, 33, 65} x packets per call in {1, k - 1, k, k + 1, 2k + 3}: every boundary of the batch's lane layout"""
    fit, bad, _ = _check(runs, k, "plain-n%d-p%d" % (n, p))
    assert fit and not bad


@pytest.mark.parametrize("k", KS)
def test_dtx_packets_carry_the_high_band_only(runs, k):
    """DTX on, speech then near-silence, 30 packets in state-continued calls of 2k+3, k+1, k, k-1, 1, ... packets"""
    fit, bad, dtx = _check(runs, k, "dtx-k%d" % k)
    assert fit and not bad
    nb = np.concatenate([runs[k]["dtx-k%d/%d/nb" % (k, i)] for i in range(len(W.plan(k, 30)))], axis=1)
    assert int((nb[:, :, 0] == 0).sum()) >= 5 * nb.shape[0]          # DTX packets did occur, in every stream
    assert dtx or not R.have_ref("fix")


@pytest.mark.parametrize("k", KS)
def test_packets_of_one_frame(runs, k):
    """framesize_ms = 20: one SILK frame and one 4-byte high-band frame per packet"""
    fit, bad, _ = _check(runs, k, "fs20-k%d" % k)
    assert fit and not bad


@pytest.mark.parametrize("k", KS)
def test_wide_band_build(runs, k):
    """the 32 kHz API rate: the kernels' second compilation"""
    fit, bad, _ = _check(runs, k, "wb-k%d" % k)
    assert fit and not bad


@pytest.mark.parametrize("k", KS)
def test_some_packets_of_a_batch_do_not_fit_their_slot(runs, k):
    """80-byte slots: status, the zeroed lengths and the untouched slots as with one coder launch per chunk"""
    fit, bad, _ = _check(runs, k, "slot-k%d" % k)
    assert fit and bad
    nb, st = runs[k]["slot-k%d/0/nb" % k], runs[k]["slot-k%d/0/st" % k]
    z = nb[:, :, 0] == 0
    for j in range(0, 2 * k + 3, k):                                   # in every batch some packets fit and some do not
        assert z[:, j:j + k].any() and (~z[:, j:j + k]).any(), j
    assert ((st == -1) == z.any(axis=1)).all() and ((st == 0) | (st == -1)).all()


@pytest.mark.parametrize("k", KS)
def test_listed_subset_of_streams(runs, k):
    """a call of every stream, then a call of 33 listed streams of 65 (map and verdict word)"""
    fit, bad, _ = _check(runs, k, "subset-k%d" % k)
    assert fit and not bad


@pytest.mark.parametrize("k", KS)
def test_two_calls_back_to_back_under_async_join(runs, k):
    """2k+3 packets, then k+1 on the continued state, nothing between them: the second call's analysis must not overrun the records the
    first call's last batch still reads"""
    fit, bad, _ = _check(runs, k, "async-k%d" % k)
    assert fit and not bad


@pytest.mark.parametrize("k", KS)
def test_launch_groups_smaller_than_the_handle(runs, k):
    """SOLO_ENC_GROUP = 32 with 65 streams: groups of 32, 32 and 1; a batch ends with its group"""
    fit, bad, _ = _check(runs, k, "group-k%d" % k)
    assert fit and not bad

"""The function-level probe of the LPC / NLSF stage functions (solo_amd/csrc/solo_fn_probe.h): record layouts, seeded case families, plain
restatements of the conditions each family must meet, and a ctypes caller of the compiled reference's exported stage functions.

Shared by tests/golden/make_fn_cases.py (the fixture generator), tests/test_fn_probe_reference.py (CPU: emulation and live reference
against the fixture, the families' conditions), tests/test_gpu_fn_probe.py (the gfx950 device bodies against the fixture) and
tools/debug/emu_coverage.py.

A GROUP is one stage function at one order: its cases are run at every call site (template instance) of that order.  Every family of a
group is a deterministic pool of input records; the generator keeps a selection of it (by what the reference does with each record) and
the fixture stores that selection and the reference's outputs.  Families whose records are built with the reference's help store the
records themselves.  Families stay inside what the product's call sites can hand the function; the preconditions are written next to each.
"""
import ctypes as C
import os
import re
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CSRC = os.path.join(ROOT, "solo_amd", "csrc")

A2NLSF, NLSF2A, MSVQ, BURG, FIND_LPC = range(5)
UNIT_NAMES = ("a2nlsf", "nlsf2a_stable", "msvq", "burg", "find_lpc")
REFUSED = -0x7FFFFFFF
HB_LPC = 8
COND_FAC_Q32 = 107374            # K_FIND_LPC_COND_FAC_Q32 (solo_consts.inc)
SURVIVORS = 16


class Build:
    """the constants of one build of the kernel source (SX_FS_KHZ 8: 16 kHz API rate, 16: 32 kHz)"""

    def __init__(self, wb):
        self.wb = bool(wb)
        self.samplerate = 32000 if wb else 16000
        self.fs = 16 if wb else 8
        self.L = 16 if wb else 10
        self.subfr = 5 * self.fs
        self.sl = self.subfr + self.L                      # a subframe with its history, as sx_find_LPC gets it
        self.hbblk = 10 * self.fs + HB_LPC
        self.xl, self.xh = 4 * self.sl, 4 * self.hbblk
        self.X = max(self.xl, self.xh)
        self.stages = 10 if wb else 6
        self.fixture = os.path.join(GOLDEN, "fn_cases_wb.npz" if wb else "fn_cases.npz")
        # group -> (unit, sites, order)
        self.groups = {
            "a2nlsf": (A2NLSF, (0, 1), self.L), "a2nlsf_hb": (A2NLSF, (2,), HB_LPC),
            "nlsf2a_stable": (NLSF2A, (0,), self.L), "nlsf2a_stable_hb": (NLSF2A, (2,), HB_LPC),
            "msvq": (MSVQ, (0,), self.L),
            "burg_0": (BURG, (0,), self.L), "burg_1": (BURG, (1,), self.L), "burg_hb": (BURG, (2,), HB_LPC),
            "find_lpc": (FIND_LPC, (0,), self.L),
        }

    def words(self, unit):
        """(in_words, out_words) of a unit's records: sx_fn_probe_words"""
        return {A2NLSF: (16, 32), NLSF2A: (16, 17), MSVQ: (52, 32), BURG: (self.X, 18), FIND_LPC: (self.X + 17, 17)}[unit]

    def burg_shape(self, site):
        """(subfr_length, nb_subfr, order) of a Burg call site"""
        return {0: (self.sl, 4, self.L), 1: (self.sl, 2, self.L), 2: (self.hbblk, 4, HB_LPC)}[site]


def fn_id(unit, site):
    return 4 * unit + site


# ---- plain integer restatements (Python ints, 32-bit wrap where the reference's arithmetic wraps) ---------------------------------------
def w32(x):
    return ((int(x) + 0x80000000) & 0xFFFFFFFF) - 0x80000000


def smulww(a, b):
    return w32((a * b) >> 16)


def rshift_round(a, s):
    return w32((a >> 1) + (a & 1)) if s == 1 else (w32((a >> (s - 1)) + 1) >> 1)


def cdiv(a, b):
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def bwexpander_32(ar, chirp_Q16):
    """SKP_Silk_bwexpander_32"""
    ar, tmp = list(ar), chirp_Q16
    for i in range(len(ar) - 1):
        ar[i] = smulww(ar[i], tmp)
        tmp = smulww(chirp_Q16, tmp)
    ar[-1] = smulww(ar[-1], tmp)
    return ar


def a2nlsf_retries(a_in, a_out):
    """How often SKP_Silk_A2NLSF expanded the bandwidth of a_in to leave a_out (retry i multiplies by the chirp 65536 - (10 + i) * i,
    SKP_Silk_A2NLSF.c:259-281; at most 30).  -1: a_out is not on that sequence."""
    cur, want = [int(v) for v in a_in], [int(v) for v in a_out]
    for r in range(31):
        if cur == want:
            return r
        if r == 30:
            break
        i = r + 1
        cur = bwexpander_32(cur, 65536 - (10 + i) * i)
    return -1


def a2nlsf_fallback(d):
    """the equally spaced vector SKP_Silk_A2NLSF gives up with"""
    step = (1 << 15) // (d + 1)
    return [step * (k + 1) for k in range(d)]


_tables = {}


def table(name, wb=False):
    """a table of the kernel source (SOLO_TAB <type> name[n] = { ... };) as a list of ints"""
    key = (name, wb)
    if key not in _tables:
        txt = open(os.path.join(CSRC, "solo_tables_wb.inc" if wb else "solo_tables.inc")).read()
        m = re.search(r"SOLO_TAB\s+\w+\s+%s\[\d+\]\s*=\s*\{([^}]*)\}" % re.escape(name), txt)
        assert m, name
        _tables[key] = [int(v, 0) for v in re.findall(r"-?\w+", m.group(1))]
    return _tables[key]


def nvec(name, wb=False):
    txt = open(os.path.join(CSRC, "solo_tables_wb.inc" if wb else "solo_tables.inc")).read()
    m = re.search(r"#define\s+%s\s*\{([^}]*)\}" % re.escape(name), txt)
    return [int(v) for v in m.group(1).split(",")]


def a2nlsf_pass(a_Q16, d):
    """ONE pass of SKP_Silk_A2NLSF's root search (no bandwidth expansion) -> (NLSF list or None where the pass fails, times the
    |ylo| >= 65536 interpolation was used, NLSF[0] forced to 0).  A plain restatement of SKP_Silk_A2NLSF.c:127-258."""
    cos = table("T_lsf_cos_Q12")
    dd = d >> 1
    P, Q = [0] * (dd + 1), [0] * (dd + 1)
    P[dd] = Q[dd] = 1 << 16
    for k in range(dd):
        P[k] = w32(-a_Q16[dd - k - 1] - a_Q16[dd + k])
        Q[k] = w32(-a_Q16[dd - k - 1] + a_Q16[dd + k])
    for k in range(dd, 0, -1):
        P[k - 1] = w32(P[k - 1] - P[k])
        Q[k - 1] = w32(Q[k - 1] + Q[k])
    for p in (P, Q):
        for k in range(2, dd + 1):
            for n in range(dd, k, -1):
                p[n - 2] = w32(p[n - 2] - p[n])
            p[k - 2] = w32(p[k - 2] - w32(p[k] << 1))

    def ev(p, x):
        y, xq = p[dd], w32(x << 4)
        for n in range(dd - 1, -1, -1):
            y = w32(p[n] + ((y * xq) >> 16))
        return y
    nlsf, big, first0 = [0] * d, 0, False
    p, xlo = P, cos[0]
    ylo = ev(p, xlo)
    root = 0
    if ylo < 0:
        first0, root, p = True, 1, Q
        ylo = ev(p, xlo)
    k = 1
    while True:
        xhi = cos[k]
        yhi = ev(p, xhi)
        if (ylo <= 0 and yhi >= 0) or (ylo >= 0 and yhi <= 0):
            ffrac = -256
            for m in range(3):
                xmid = rshift_round(xlo + xhi, 1)
                ymid = ev(p, xmid)
                if (ylo <= 0 and ymid >= 0) or (ylo >= 0 and ymid <= 0):
                    xhi, yhi = xmid, ymid
                else:
                    xlo, ylo = xmid, ymid
                    ffrac += 128 >> m
            if abs(ylo) < 65536:
                den = ylo - yhi
                if den != 0:
                    ffrac += cdiv(w32(ylo << 5) + (den >> 1), den)
            else:
                big += 1
                den = (ylo - yhi) >> 5
                if den == 0:
                    return None, big, first0
                ffrac += cdiv(ylo, den)
            nlsf[root] = min((k << 8) + ffrac, 32767)
            root += 1
            if root >= d:
                return nlsf, big, first0
            p = Q if root & 1 else P
            xlo = cos[k - 1]
            ylo = w32((1 - (root & 2)) << 12)
        else:
            k += 1
            xlo, ylo = xhi, yhi
            if k > 128:
                return None, big, first0


def a2nlsf_full(a_Q16, d):
    """SKP_Silk_A2NLSF restated with a2nlsf_pass -> (NLSF, a_Q16 as it is left, retries, uses of the |ylo| >= 65536 interpolation in the
    passes that failed, the same in the pass that succeeded (0 after a fall-back))"""
    a, big_failed = [int(v) for v in a_Q16[:d]], 0
    for i in range(31):
        nl, big, _ = a2nlsf_pass(a, d)
        if nl is not None:
            return nl, a, i, big_failed, big
        big_failed += big
        if i == 30:
            break
        a = bwexpander_32(a, 65536 - (10 + i + 1) * (i + 1))
    return a2nlsf_fallback(d), a, 30, big_failed, 0


def nlsf2a_a32(nlsf, d):
    """SKP_Silk_NLSF2A up to its limiter (SKP_Silk_NLSF2A.c:59-92) -> the d coefficients in Q12 BEFORE they are limited to int16"""
    cos = table("T_lsf_cos_Q12")
    c = []
    for k in range(d):
        fi = nlsf[k] >> 8
        ff = nlsf[k] - (fi << 8)
        c.append(w32((cos[fi] << 8) + (cos[fi + 1] - cos[fi]) * ff))
    dd = d >> 1

    def rr64(v, s):
        return ((v >> (s - 1)) + 1) >> 1

    def poly(cl):
        out = [0] * (dd + 1)
        out[0], out[1] = 1 << 20, w32(-cl[0])
        for k in range(1, dd):
            f = cl[2 * k]
            out[k + 1] = w32((out[k - 1] << 1) - w32(rr64(f * out[k], 20)))
            for n in range(k, 1, -1):
                out[n] = w32(out[n] + w32(out[n - 2] - w32(rr64(f * out[n - 1], 20))))
            out[1] = w32(out[1] - f)
        return out
    P, Q = poly(c[0:]), poly(c[1:])
    a = [0] * d
    for k in range(dd):
        pt, qt = w32(P[k + 1] + P[k]), w32(Q[k + 1] - Q[k])
        a[k] = w32(-rshift_round(w32(pt + qt), 9))
        a[d - k - 1] = rshift_round(w32(qt - pt), 9)
    return a


def nlsf2a_limit(a32):
    """the limiter of SKP_Silk_NLSF2A (SKP_Silk_NLSF2A.c:93-118) -> (coefficients, rounds of bandwidth expansion, saturated after 10 rounds)"""
    a, d = list(a32), len(a32)
    for i in range(10):
        mx, idx = 0, 0
        for k in range(d):
            if abs(a[k]) > mx:
                mx, idx = abs(a[k]), k
        if mx <= 32767:
            return a, i, False
        mx = min(mx, 98369)
        sc = 65470 - cdiv((65470 >> 2) * (mx - 32767), (mx * (idx + 1)) >> 2)
        a = bwexpander_32(a, sc)
    return [max(-32768, min(32767, v)) for v in a], 10, True


def weights_laroia(nlsf, d):
    """SKP_Silk_NLSF_VQ_weights_laroia"""
    w = [0] * d
    t1 = (1 << 21) // max(nlsf[0], 3)
    t2 = (1 << 21) // max(nlsf[1] - nlsf[0], 3)
    w[0] = min(t1 + t2, 32767)
    for k in range(1, d - 1, 2):
        t1 = (1 << 21) // max(nlsf[k + 1] - nlsf[k], 3)
        w[k] = min(t1 + t2, 32767)
        t2 = (1 << 21) // max(nlsf[k + 2] - nlsf[k + 1], 3)
        w[k + 1] = min(t1 + t2, 32767)
    t1 = (1 << 21) // max((1 << 15) - nlsf[d - 1], 3)
    w[d - 1] = min(t1 + t2, 32767)
    return w


def sum_sqr_shift(x):
    """SKP_Silk_sum_sqr_shift on a 4-byte aligned vector -> (energy, shift)"""
    x = [int(v) for v in x]
    n, i, nrg, shft = len(x) - 1, 0, 0, 0
    while i < n:
        nrg = w32(nrg + x[i] * x[i])
        nrg = w32(nrg + x[i + 1] * x[i + 1])
        i += 2
        if nrg < 0:
            nrg, shft = (nrg & 0xFFFFFFFF) >> 2, 2
            break
    while i < n:
        t = w32(x[i] * x[i] + x[i + 1] * x[i + 1])
        nrg = w32((nrg & 0xFFFFFFFF) + ((t & 0xFFFFFFFF) >> shft))
        if nrg < 0:
            nrg, shft = (nrg & 0xFFFFFFFF) >> 2, shft + 2
        i += 2
    if i == n:
        nrg = w32((nrg & 0xFFFFFFFF) + (((x[i] * x[i]) & 0xFFFFFFFF) >> shft))
    if nrg & 0xC0000000:
        nrg, shft = (nrg & 0xFFFFFFFF) >> 2, shft + 2
    return nrg, shft


def msvq_stage0_rd(build, nlsf, W, sigtype, mu):
    """rate-distortion values of the first stage of SKP_Silk_NLSF_MSVQ_encode_FIX (SKP_Silk_NLSF_VQ_rate_distortion_FIX with one input
    vector): int64 numpy [K]"""
    pre = "T_nlsf16_cb%d" if build.wb else "T_nlsf_cb%d"
    K = nvec(("T_NLSF16_CB%d_NVEC" if build.wb else "T_NLSF_CB%d_NVEC") % sigtype, build.wb)[0]
    cb = np.array(table((pre + "_Q15") % sigtype, build.wb)[:K * build.L], np.int64).reshape(K, build.L)
    rates = np.array(table((pre + "_rates_Q5") % sigtype, build.wb)[:K], np.int64)
    diff = np.asarray(nlsf, np.int64)[None, :build.L] - cb
    d16 = ((diff + 32768) & 0xFFFF) - 32768
    err = np.zeros(K, np.int64)
    w16 = ((np.asarray(W, np.int64)[:build.L] + 32768) & 0xFFFF) - 32768
    for m in range(build.L):
        err = err + ((d16[:, m] * d16[:, m] * w16[m]) >> 16)
    return err + (((rates + 32768) & 0xFFFF) - 32768) * int(mu)


def msvq_mu(sigtype, sa_Q8, sparse_Q8):
    """(NLSF_mu_Q15, NLSF_mu_fluc_red_Q16) as SKP_Silk_process_NLSFs_FIX derives them from the speech activity and the sparseness"""
    def smlawb(acc, a, b):
        return w32(acc + ((a * (((b + 32768) & 0xFFFF) - 32768)) >> 16))
    if sigtype == 0:
        mu, fl = smlawb(66, -8388, sa_Q8), smlawb(6554, -838848, sa_Q8)
    else:
        mu, fl = smlawb(164, -33554, sa_Q8), smlawb(13107, -1677696, sa_Q8 + sparse_Q8)
    return max(mu, 1), fl


# ---- case families ------------------------------------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _sorted_nlsf(rng, n, d, lo=1, hi=32767):
    return np.sort(rng.integers(lo, hi + 1, (n, d)), axis=1).astype(np.int32)


def _pad16(v):
    out = np.zeros((v.shape[0], 16), np.int32)
    out[:, :v.shape[1]] = v
    return out


A_Q16_MAX = 1 << 22     # |a_Q16| the call sites can hand sx_a2nlsf: Burg keeps its coefficients as int32 in Q25 and hands them over >> 9


def a2nlsf_pool(build, d, family, ref=None):
    """a2nlsf records (int32 [n, 16]).  Precondition of the call sites: |a_Q16| < 2^22 (A_Q16_MAX)."""
    rng = _rng("a2nlsf", d, family)
    n = 1200 if family in ("uniform_65536", "uniform_4194304") else 3000
    if family == "nlsf_filters":            # stable filters: random sorted NLSFs through the reference's SKP_Silk_NLSF2A, << 4 (stored in the fixture)
        nl = _sorted_nlsf(rng, n, d)
        return _pad16(np.stack([ref.nlsf2a(v, d) for v in nl]).astype(np.int32) << 4)
    if family == "uniform_20000":
        return _pad16(rng.integers(-19999, 20000, (n, d)).astype(np.int32))
    if family == "uniform_65536":
        return _pad16(rng.integers(-65535, 65536, (n, d)).astype(np.int32))
    if family == "uniform_4194304":         # the whole domain: steep polynomials, whose roots are interpolated from |ylo| >= 65536
        return _pad16(rng.integers(-A_Q16_MAX + 1, A_Q16_MAX, (n, d)).astype(np.int32))
    if family == "sections":                # products of second-order sections of radius 0.98 .. 1.02, a cluster of them near-identical
        out, n = [], 1500                   # (order 16: eight near-identical sections leave the domain, (1 + z^-2)^8 has a coefficient of 70)
        for _ in range(200000):
            th0, cluster = rng.uniform(0.05, np.pi - 0.05), int(rng.integers(2, d // 2 + 1))
            poly = np.ones(1)
            for s in range(d // 2):
                r, th = rng.uniform(0.98, 1.02), (th0 + rng.normal(0.0, 0.02) if s < cluster else rng.uniform(0.05, np.pi - 0.05))
                poly = np.convolve(poly, [1.0, -2.0 * r * np.cos(th), r * r])
            a = np.rint(-poly[1:] * 65536.0)
            if np.abs(a).max() < A_Q16_MAX:
                out.append(a.astype(np.int32))
                if len(out) == n:
                    break
        assert len(out) == n
        return _pad16(np.stack(out))
    raise KeyError(family)


A2NLSF_FAMILIES = ("nlsf_filters", "uniform_20000", "uniform_65536", "uniform_4194304", "sections")
A2NLSF_CLASSES = ("no_retry", "retries_1_5", "retries_6_30", "fallback", "first_root_0")
A2NLSF_BIG = "big_ylo"          # the |ylo| >= 65536 interpolation in the pass that succeeds (found with a2nlsf_full: not visible in the outputs)


def a2nlsf_class(a_in, out, d):
    """-> (retries, set of the classes of A2NLSF_CLASSES a case belongs to), from the reference's outputs alone"""
    nl, a_out = [int(v) for v in out[:d]], out[16:16 + d]
    r = a2nlsf_retries(a_in[:d], a_out)
    fb = nl == a2nlsf_fallback(d) and a2nlsf_pass([int(v) for v in a_out], d)[0] is None      # (gave up: the pass over what it left fails too)
    cls = set()
    if fb:
        cls.add("fallback")
    elif r == 0:
        cls.add("no_retry")
    elif 1 <= r <= 5:
        cls.add("retries_1_5")
    elif r > 5:
        cls.add("retries_6_30")
    if nl[0] == 0 and not fb:
        cls.add("first_root_0")
    return r, cls


NLSF2A_FAMILIES = ("sorted", "close_neighbours", "clusters_low", "clusters_high", "runs_of_equal", "two_clusters")
NLSF2A_CLASSES = ("ordinary", "limiter", "saturated", "unstable", "zero_fallback")


def nlsf2a_pool(build, d, family):
    """nlsf2a_stable records (int32 [n, 16]).  Precondition of the call sites: every value in 0 .. 32767, non-decreasing."""
    rng = _rng("nlsf2a", d, family)
    n = 4000
    if family == "sorted":
        v = _sorted_nlsf(rng, n, d)
    elif family == "close_neighbours":      # neighbours 1 .. 3 apart somewhere in a sorted vector
        v = _sorted_nlsf(rng, n, d)
        for i in range(n):
            for _ in range(int(rng.integers(1, d // 2 + 1))):
                k = int(rng.integers(0, d - 1))
                v[i, k + 1] = min(32767, v[i, k] + int(rng.integers(1, 4)))
        v = np.sort(v, axis=1)
    elif family in ("clusters_low", "clusters_high"):      # all of it within a few hundred of one end, steps of 0 .. 3 and a few larger ones
        steps = rng.integers(0, 4, (n, d)) + (rng.random((n, d)) < 0.2) * rng.integers(0, 400, (n, d))
        v = np.cumsum(steps, axis=1) + rng.integers(0, 40, (n, 1))
        v = np.clip(v if family == "clusters_low" else 32767 - v[:, ::-1], 0, 32767)
    elif family == "runs_of_equal":         # runs of equal values (the interpolation of two vectors can produce them)
        v = _sorted_nlsf(rng, n, d, 0)
        for i in range(n):
            k, ln = int(rng.integers(0, d - 1)), int(rng.integers(2, d + 1))
            v[i, k:k + ln] = v[i, k]
        v = np.sort(v, axis=1)
    elif family == "two_clusters":          # half of the values crowded at each end
        h = d // 2
        lo = np.cumsum(rng.integers(0, 6, (n, h)), axis=1) + rng.integers(0, 200, (n, 1))
        hi = 32767 - np.cumsum(rng.integers(0, 6, (n, d - h)), axis=1)[:, ::-1] - rng.integers(0, 200, (n, 1))
        v = np.clip(np.concatenate([lo, hi], axis=1), 0, 32767)
    else:
        raise KeyError(family)
    return _pad16(np.ascontiguousarray(v).astype(np.int32))


def nlsf2a_class(nlsf, d, unstable_first, out):
    """classes of NLSF2A_CLASSES of a case.  unstable_first: the reference's SKP_Silk_LPC_inverse_pred_gain on the reference's
    SKP_Silk_NLSF2A output said unstable; out: the reference's SKP_Silk_NLSF2A_stable output.  The limiter is read off the restatement
    nlsf2a_a32 / nlsf2a_limit (which the generator checks against the reference's SKP_Silk_NLSF2A case by case)."""
    a32 = nlsf2a_a32([int(v) for v in nlsf[:d]], d)
    lim, rounds, sat = nlsf2a_limit(a32)
    cls = set()
    if rounds > 0:
        cls.add("limiter")
    if sat:
        cls.add("saturated")
    if unstable_first:
        cls.add("unstable")
        if not any(int(v) for v in out[:d]) and any(lim):
            cls.add("zero_fallback")
    if not cls:
        cls.add("ordinary")
    return cls


def _i16(x):
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


_pcm = {}


def _pcm_family(name):
    """a family of tests/burg_sites_inputs.py as int16 [64, 3840]"""
    if name not in _pcm:
        import burg_sites_inputs as B
        _pcm[name] = B.family(name).reshape(B.N, -1)
    return _pcm[name]


BURG_FAMILIES = ("silence", "lsb_noise", "white_full_scale", "square_full_scale", "speech_like", "sinusoid", "two_tone", "silence_then_full_scale",
                 "nyquist_full_scale", "alternation", "periodic", "dc_full_scale", "impulses", "level_sweep")


def burg_pool(build, site, family):
    """Burg records (int32 [n, X], one sample per word): the families of tests/burg_sites_inputs.py cut to the site's block shape (nb_subfr
    blocks of subfr_length samples, contiguous), plus full-scale alternations, exactly periodic blocks, DC and isolated impulses."""
    import burg_sites_inputs as B
    sl, nb, D = build.burg_shape(site)
    n_s = sl * nb
    rng = _rng("burg", build.wb, site, family)
    n = 80                                  # (13 families of 80 and one of 240: 3 x 1280 = 3840 cases of the unit per build)
    if family in B.FAMILIES:
        pcm = _pcm_family(family)                                      # [64, 3840]
        offs = rng.integers(0, pcm.shape[1] - n_s, n)
        if family == "silence_then_full_scale":                          # cut across the onset
            offs = 2 * 640 - rng.integers(0, n_s, n)
        x = np.stack([pcm[i % B.N, o:o + n_s] for i, o in enumerate(offs)])
    elif family == "alternation":           # +A, -A, ... at full scale and just below, whole record or from some block on
        x = np.zeros((n, n_s), np.int16)
        for i in range(n):
            A = 32767 - int(rng.integers(0, 3)) * (i % 7)
            v = A * (1 - 2 * (np.arange(n_s) % 2))
            if i % 3 == 1:
                v = -v
            if i % 3 == 2:
                v[:int(rng.integers(0, nb)) * sl] = 0
            x[i] = _i16(v)
    elif family == "periodic":              # exactly periodic blocks: period 1 .. 2 D, full scale to a few LSB
        x = np.zeros((n, n_s), np.int16)
        for i in range(n):
            per = 1 + i % (2 * D)
            amp = (32767, 32767, 20000, 3000, 100, 3)[i % 6]
            cyc = rng.integers(-amp, amp + 1, per)
            x[i] = _i16(np.resize(cyc, n_s))
    elif family == "dc_full_scale":
        x = np.stack([np.full(n_s, (32767, -32768, 32766, -32767, 16384, 1)[i % 6] - (i // 6 if i % 6 == 0 else 0), np.int16) for i in range(n)])
    elif family == "level_sweep":           # alternations, DC and square waves of period 2 .. 58 over the whole range of levels
        n, t = 240, np.arange(n_s)
        x = np.zeros((n, n_s), np.int16)
        for i in range(n):
            A = (1, 2, 3, 5, 9, 17, 40, 100, 331, 1000, 3000, 9000, 16384, 25000, 32767)[i % 15] + (i // 45)
            x[i] = _i16((A * (1 - 2 * (t % 2)), np.full(n_s, A), A * (1 - 2 * ((t // (1 + i // 15 * 2)) % 2)))[(i // 15) % 3])
    elif family == "impulses":
        x = np.zeros((n, n_s), np.int16)
        for i in range(n):
            x[i, rng.integers(0, n_s, 1 + i % 5)] = rng.integers(-32768, 32768, 1 + i % 5)
    else:
        raise KeyError(family)
    out = np.zeros((n, build.X), np.int32)
    out[:, :n_s] = x
    return out


def burg_rshifts(x):
    """the scaling Burg starts from: SKP_Silk_sum_sqr_shift's shift of the whole record (the MAX_RSHIFTS clamp acts above 7)"""
    return sum_sqr_shift(x)[1]


_count_libs = {}


def count_lib(build):
    """the host emulation compiled with -DSX_BURG_COUNT -DSX_DOT_COUNT into build/ (rebuilt when a source is newer): the same code with
    counters at branches that the outputs do not show (solo_enc_analysis.h, solo_fix.h)"""
    import glob
    import subprocess
    if build.wb not in _count_libs:
        path = os.path.join(ROOT, "build", "libsolo_emu_count%s.so" % ("_wb" if build.wb else ""))
        src = os.path.join(ROOT, "tests", "emu", "solo_emu.cpp")
        deps = [src] + glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.inc"))
        if not os.path.exists(path) or any(os.path.getmtime(d) > os.path.getmtime(path) for d in deps):
            os.makedirs(os.path.dirname(path), exist_ok=True)
            subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-fwrapv", "-fno-strict-aliasing", "-w", "-DSOLO_HOST_EMU", "-DSX_BURG_COUNT",
                                   "-DSX_DOT_COUNT"] + (["-DSX_FS_KHZ=16"] if build.wb else []) + [src, "-o", path + ".tmp%d" % os.getpid()])
            os.replace(path + ".tmp%d" % os.getpid(), path)
        lib = C.CDLL(path)
        lib.emu_fn.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        _count_libs[build.wb] = lib
    return _count_libs[build.wb]


def _counted(build, unit, site, recs, symbol, n_counters, pick):
    """records one by one through the counting build -> int64 [n, len(pick)]: by how much the counters `pick` of `symbol` rose in each"""
    lib = count_lib(build)
    count = (C.c_longlong * n_counters).in_dll(lib, symbol)
    iw, ow = build.words(unit)
    out, got = np.zeros(ow, np.int32), np.zeros((len(recs), len(pick)), np.int64)
    for i, r in enumerate(np.ascontiguousarray(recs, np.int32)):
        before = [count[k] for k in pick]
        assert lib.emu_fn(fn_id(unit, site), 1, r.ctypes.data_as(C.c_void_p), iw, out.ctypes.data_as(C.c_void_p), ow) == 0
        got[i] = [count[k] - b for k, b in zip(pick, before)]
    return got


def burg_exits(build, site, recs):
    """which records leave the Burg recursion through the |num| >= den exit -> bool [n] (counter [site][2] of SX_BURG_COUNT); the outputs
    alone do not show it: a vector that is zero from some order on may also be an honest result"""
    return _counted(build, BURG, site, recs, "sx_burg_count", 12, [4 * site + 2])[:, 0] > 0


def find_lpc_shifts(build, recs):
    """per record, how often sx_find_LPC took each arm of its two energy alignments -> int64 [n, 4]: first shift >= 0, < 0 (the second-half
    run of Burg against the whole-frame run), a candidate's rshift0 >= rshift1, < (counters 11 .. 14 of SX_DOT_COUNT)"""
    return _counted(build, FIND_LPC, 0, recs, "sx_dot_count", 16, [11, 12, 13, 14])


def burg_exit_order(A_Q16, d):
    """trailing coefficients that are exactly zero: what the |num| >= den exit leaves behind (SKP_Silk_burg_modified.c: the remaining
    coefficients stay 0); d for an all-zero vector"""
    k = 0
    while k < d and int(A_Q16[d - 1 - k]) == 0:
        k += 1
    return k


FIND_LPC_FAMILIES = ("speech_like", "speech_quiet", "white_full_scale", "square_full_scale", "sinusoid", "lsb_noise", "step_up", "step_down", "silence", "two_spectra")


def find_lpc_pool(build, family):
    """find_lpc records (int32 [n, X + 17]): four subframes with their history, the previous quantised NLSFs (a stage vector of the
    codebook or a sorted random vector), useInterp 0 / 1"""
    import burg_sites_inputs as B
    rng = _rng("find_lpc", build.wb, family)
    n, n_s = 160, build.xl
    if family == "two_spectra":
        # noise through the all-pole filter of one NLSF vector in the frame's first half and of another in its second; the previous NLSFs
        # are a vector from which the first half's lies 0, 1/4, 1/2 or 3/4 of the way to the second's: every interpolation index can win
        L, out = build.L, np.zeros((2 * n, build.X + 17), np.int32)

        def lpc(nl):
            w = np.pi * np.asarray(nl, float) / 32768.0
            P, Q = np.array([1.0, 1.0]), np.array([1.0, -1.0])
            for k in range(L):
                sec = [1.0, -2.0 * np.cos(w[k]), 1.0]
                P, Q = (np.convolve(P, sec), Q) if k % 2 == 0 else (P, np.convolve(Q, sec))
            return (0.5 * (P + Q))[:L + 1]

        def colour(a, m):       # a [rows, L + 1] -> coloured noise of root mean square 4096 [rows, m]; integer arithmetic (all rows filtered in step)
            aq = np.rint(a[:, 1:] * (1 << 20)).astype(np.int64)
            e, y = rng.integers(-4096, 4097, (len(a), m + 300)), np.zeros((len(a), m + 300 + L), np.int64)
            for t in range(m + 300):
                y[:, t + L] = np.clip(e[:, t] - ((aq * y[:, t:t + L][:, ::-1]).sum(axis=1) >> 20), -(1 << 40), 1 << 40)
            y = y[:, L + 300:]
            rms = np.sqrt((y.astype(float) ** 2).mean(axis=1, keepdims=True))
            return (y << 12) // np.maximum(rms.astype(np.int64), 1)
        nA = np.sort(32768.0 * (np.arange(1, L + 1) + rng.uniform(-0.35, 0.35, (2 * n, L))) / (L + 1), axis=1)
        nB = np.sort(32768.0 * (np.arange(1, L + 1) + rng.uniform(-0.35, 0.35, (2 * n, L))) / (L + 1), axis=1)
        f = (np.arange(2 * n) % 4)[:, None] / 4.0
        amp = np.array((3000, 300, 12000))[(np.arange(2 * n) // 4) % 3][:, None]
        x = np.concatenate([colour(np.stack([lpc(v) for v in nA + f * (nB - nA)]), 2 * build.sl), colour(np.stack([lpc(v) for v in nB]), 2 * build.sl)], axis=1)
        out[:, :n_s] = np.clip((x * amp) >> 12, -32768, 32767)
        out[:, build.X:build.X + L] = np.rint(nA)
        out[:, build.X + 16] = 1
        return out
    base = {"speech_quiet": "speech_like", "step_up": "white_full_scale", "step_down": "white_full_scale"}.get(family, family)
    pcm = _pcm_family(base)
    offs = rng.integers(0, pcm.shape[1] - n_s, n)
    x = np.stack([pcm[i % B.N, o:o + n_s] for i, o in enumerate(offs)]).astype(np.int32)
    if family == "speech_quiet":
        x = x >> rng.integers(4, 12, (n, 1))
    if family in ("step_up", "step_down"):      # one half of the frame's first two subframes far below the other: the two residual energies get different shifts
        quiet = np.arange(n_s)[None, :] // build.sl == (0 if family == "step_up" else 1)
        sh = rng.integers(6, 15, (n, 1))
        x = np.where(quiet | (np.arange(n_s)[None, :] // build.sl >= 2) & (rng.random((n, 1)) < 0.5), x >> sh, x)
    out = np.zeros((n, build.X + 17), np.int32)
    out[:, :n_s] = x
    out[:, build.X:build.X + build.L] = _sorted_nlsf(rng, n, build.L, 200, 32000)
    out[:, build.X + 16] = np.arange(n) % 4 != 0
    return out


MSVQ_FAMILIES = ("around_codebook", "midpoints", "far")


def msvq_pool(build, family, n=None):
    """msvq records (int32 [n, 52]): a sorted target, the previous quantised vector, Laroia weights of the target, the signal type, the two
    rate weights from a drawn speech activity / sparseness, deactivate_fluc_red.  around_codebook: sums of one vector per stage (a path
    through the codebook) plus noise; midpoints: midpoints of two first-stage vectors of equal rate, single coordinates nudged
    until the two rate-distortion values tie exactly; far: sorted random vectors."""
    rng = _rng("msvq", build.wb, family)
    n = n or (1500 if family == "midpoints" else 600)
    L = build.L
    out = np.zeros((n, 52), np.int32)
    for i in range(n):
        sig = int(rng.integers(0, 2))
        pre = ("T_nlsf16_cb%d" if build.wb else "T_nlsf_cb%d") % sig
        nv = nvec(("T_NLSF16_CB%d_NVEC" if build.wb else "T_NLSF_CB%d_NVEC") % sig, build.wb)
        cb = np.array(table(pre + "_Q15", build.wb), np.int64).reshape(-1, L)
        rates = table(pre + "_rates_Q5", build.wb)
        base = np.cumsum([0] + nv[:-1])
        path = [int(rng.integers(0, k)) for k in nv]

        def vec(p):
            return sum(cb[base[s] + p[s]] for s in range(len(nv)))
        if family == "around_codebook":
            t = vec(path) + np.rint(rng.normal(0.0, rng.choice([0.0, 20.0, 150.0]), L)).astype(np.int64)
            prev = vec([int(rng.integers(0, k)) for k in nv])
        elif family == "midpoints":
            same = [j for j in range(nv[0]) if rates[j] == rates[path[0]] and j != path[0]]
            j = int(rng.choice(same)) if same else path[0]
            s2 = cb[path[0]] + cb[j]
            t = np.sort(np.clip((s2 + rng.integers(0, 2, L) * (s2 & 1)) // 2, 1, 32767))
            prev = vec(path)

            def gap(tt):        # difference of the two vectors' weighted errors (their rates are equal: a tie of the rate-distortion value at 0)
                ww = weights_laroia([int(v) for v in tt], L)
                return sum((((int(tt[m]) - int(cb[path[0]][m])) ** 2 * ww[m]) >> 16) - (((int(tt[m]) - int(cb[j][m])) ** 2 * ww[m]) >> 16) for m in range(L))
            g = gap(t)
            for _ in range(80):     # nudge single coordinates towards the tie
                if g == 0:
                    break
                t2 = t.copy()
                t2[int(rng.integers(0, L))] += int(rng.choice([-2, -1, 1, 2]))
                if t2.min() < 1 or t2.max() > 32767 or (np.diff(t2) < 0).any():
                    continue
                g2 = gap(t2)
                if abs(g2) < abs(g):
                    t, g = t2, g2
        else:
            t = np.sort(rng.integers(1, 32768, L))
            prev = np.sort(rng.integers(1, 32768, L))
        t = np.sort(np.clip(t, 1, 32767))
        prev = np.sort(np.clip(prev, 1, 32767))
        mu, fl = msvq_mu(sig, int(rng.integers(0, 257)), int(rng.integers(0, 257)))
        out[i, :L], out[i, 16:16 + L], out[i, 32:32 + L] = t, prev, weights_laroia([int(v) for v in t], L)
        out[i, 48:52] = (sig, mu, fl, int(rng.integers(0, 4) == 0))
    return out


def msvq_stage0_tie(build, rec):
    """an exact tie of the rate-distortion value among the best cur_survivors + 1 entries of the first stage (numpy restatement)"""
    rd = np.sort(msvq_stage0_rd(build, rec[:16], rec[32:48], int(rec[48]), int(rec[49])))[:SURVIVORS + 1]
    return bool((np.diff(rd) == 0).any())


def msvq_stage0_cut(build, rec):
    """the relative rate-distortion rule cuts the first stage's survivors to min_survivors (SKP_Silk_NLSF_MSVQ_encode_FIX.c: threshold =
    (1 + 16 * 0.1) * best; survivors above it go while more than 8 are left)"""
    rd = np.sort(msvq_stage0_rd(build, rec[:16], rec[32:48], int(rec[48]), int(rec[49])))
    cur = min(SURVIVORS, len(rd))
    best = int(rd[0])
    if best >= 0x7FFFFFFF // 16:
        return False
    thr = w32(best + ((w32(SURVIVORS * best) * 6554) >> 16))
    while int(rd[cur - 1]) > thr and cur > SURVIVORS // 2:
        cur -= 1
    return cur == SURVIVORS // 2


# ---- the compiled reference's stage functions through ctypes ---------------------------------------------------------------------------
class Ref:
    """SKP_Silk_A2NLSF, SKP_Silk_NLSF2A(_stable), SKP_Silk_LPC_inverse_pred_gain, SKP_Silk_NLSF_MSVQ_encode_FIX, SKP_Silk_NLSF_VQ_weights_laroia,
    SKP_Silk_burg_modified and SKP_Silk_find_LPC_FIX of oracle/_ref/libsolo_ref_<kind>.so (kind: fix = -O2, fix_O3): plain exported symbols"""

    def __init__(self, kind="fix"):
        import sys
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import refcodec as R
        lib = C.CDLL(R.ref_lib_path(kind))
        p, i = C.c_void_p, C.c_int          # (pointers as pointers: the default would truncate 64-bit addresses)
        for name, args in (("SKP_Silk_A2NLSF", [p, p, i]), ("SKP_Silk_NLSF2A", [p, p, i]), ("SKP_Silk_NLSF2A_stable", [p, p, i]),
                           ("SKP_Silk_LPC_inverse_pred_gain", [p, p, i]), ("SKP_Silk_NLSF_VQ_weights_laroia", [p, p, i]),
                           ("SKP_Silk_NLSF_MSVQ_encode_FIX", [p, p, p, p, p, i, i, i, i, i]), ("SKP_Silk_burg_modified", [p, p, p, p, i, i, C.c_int32, i]),
                           ("SKP_Silk_find_LPC_FIX", [p, p, p, i, i, p, i])):
            f = getattr(lib, name)
            f.argtypes = args
            f.restype = i if name == "SKP_Silk_LPC_inverse_pred_gain" else None
        self.lib = lib

    @staticmethod
    def _p(a):
        return a.ctypes.data_as(C.c_void_p)

    def a2nlsf(self, a_Q16, d):
        a, nl = np.ascontiguousarray(a_Q16[:16], np.int32).copy(), np.zeros(16, np.int32)
        self.lib.SKP_Silk_A2NLSF(self._p(nl), self._p(a), d)
        nl[d:], a[d:] = 0, 0
        return np.concatenate([nl, a])

    def nlsf2a(self, nlsf, d):
        v, a = np.ascontiguousarray(nlsf[:16], np.int32).copy(), np.zeros(16, np.int16)
        self.lib.SKP_Silk_NLSF2A(self._p(a), self._p(v), d)
        return a[:d].astype(np.int32)

    def unstable(self, a_Q12, d):
        a, g = np.zeros(16, np.int16), np.zeros(1, np.int32)
        a[:d] = a_Q12[:d]
        return int(self.lib.SKP_Silk_LPC_inverse_pred_gain(self._p(g), self._p(a), d)) == 1

    def nlsf2a_stable(self, nlsf, d):
        v, a = np.zeros(16, np.int32), np.zeros(16, np.int16)
        v[:d] = nlsf[:d]
        self.lib.SKP_Silk_NLSF2A_stable(self._p(a), self._p(v), d)
        out = np.zeros(17, np.int32)
        out[:d] = a[:d]
        out[16] = 1 if self.unstable(self.nlsf2a(v, d), d) or max(abs(t) for t in nlsf2a_a32([int(t) for t in v[:d]], d)) > 32767 else 0
        return out

    def weights(self, nlsf, d):
        v, w = np.ascontiguousarray(nlsf[:16], np.int32).copy(), np.zeros(16, np.int32)
        self.lib.SKP_Silk_NLSF_VQ_weights_laroia(self._p(w), self._p(v), d)
        return w[:d]

    def msvq(self, rec, L):
        nl, prev, W = (np.ascontiguousarray(rec[o:o + 16], np.int32).copy() for o in (0, 16, 32))
        idx = np.zeros(16, np.int32)
        cb = C.addressof(C.c_char.in_dll(self.lib, "SKP_Silk_NLSF_CB%d_%d" % (int(rec[48]), L)))
        self.lib.SKP_Silk_NLSF_MSVQ_encode_FIX(self._p(idx), self._p(nl), cb, self._p(prev), self._p(W), int(rec[49]), int(rec[50]), SURVIVORS, L, int(rec[51]))
        nl[L:] = 0
        return np.concatenate([idx, nl])

    def burg(self, x, sl, nb, D):
        xs = np.ascontiguousarray(x[:sl * nb]).astype(np.int16)
        e, q, A = np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(16, np.int32)
        self.lib.SKP_Silk_burg_modified(self._p(e), self._p(q), self._p(A), self._p(xs), sl, nb, COND_FAC_Q32, D)
        A[D:] = 0
        return np.concatenate([e, q, A])

    def find_lpc(self, rec, build):
        xs = np.ascontiguousarray(rec[:build.xl]).astype(np.int16)
        prev = np.ascontiguousarray(rec[build.X:build.X + 16], np.int32).copy()
        nl, ii = np.zeros(16, np.int32), np.zeros(1, np.int32)
        self.lib.SKP_Silk_find_LPC_FIX(self._p(nl), self._p(ii), self._p(prev), 1 if int(rec[build.X + 16]) == 1 else 0, build.L, self._p(xs), build.sl)
        nl[build.L:] = 0
        return np.concatenate([nl, ii])

    def run(self, build, group, rec):
        """one record of a group through the reference -> its output record (the a2nlsf / burg outputs do not depend on the site)"""
        unit, sites, d = build.groups[group]
        if unit == A2NLSF:
            return self.a2nlsf(rec, d)
        if unit == NLSF2A:
            return self.nlsf2a_stable(rec, d)
        if unit == MSVQ:
            return self.msvq(rec, d)
        if unit == BURG:
            return self.burg(rec, *build.burg_shape(sites[0]))
        return self.find_lpc(rec, build)


def run_ref(build, group, recs, kind="fix", fork=True):
    """every record of recs through the reference -> (out int32 [n, out_words], ok bool [n]).  fork: in forked children, a record on which
    the reference dies (it divides by zero on some extreme inputs) is marked not ok and the rest goes on in a fresh child."""
    import mmap
    n, ow = len(recs), build.words(build.groups[group][0])[1]
    if not fork:
        ref = Ref(kind)
        return np.stack([ref.run(build, group, r) for r in recs]).astype(np.int32).reshape(n, ow), np.ones(n, bool)
    mm = mmap.mmap(-1, max(1, n * (ow + 1) * 4))
    sh = np.frombuffer(mm, np.int32, n * (ow + 1)).reshape(n, ow + 1)
    sh[:] = 0
    start = 0
    while start < n:
        pid = os.fork()
        if pid == 0:
            try:
                ref = Ref(kind)
                for i in range(start, n):
                    sh[i, :ow] = ref.run(build, group, recs[i])
                    sh[i, ow] = 1
            finally:
                os._exit(0)
        os.waitpid(pid, 0)
        undone = np.nonzero(sh[start:, ow] == 0)[0]
        if len(undone) == 0:
            break
        start += int(undone[0]) + 1
    out, ok = sh[:, :ow].copy(), sh[:, ow] == 1
    del sh
    return out, ok


# ---- the fixture ----------------------------------------------------------------------------------------------------------------------
GROUP_FAMILIES = {"a2nlsf": A2NLSF_FAMILIES, "a2nlsf_hb": A2NLSF_FAMILIES, "nlsf2a_stable": NLSF2A_FAMILIES, "nlsf2a_stable_hb": NLSF2A_FAMILIES,
                  "msvq": MSVQ_FAMILIES, "burg_0": BURG_FAMILIES, "burg_1": BURG_FAMILIES, "burg_hb": BURG_FAMILIES, "find_lpc": FIND_LPC_FAMILIES}
# families whose records are kept in the fixture: they need the reference, or come out of a long search
STORED = {("a2nlsf", "nlsf_filters"), ("a2nlsf_hb", "nlsf_filters"), ("msvq", "midpoints")}


def pool(build, group, family, ref=None):
    unit, sites, d = build.groups[group]
    if unit == A2NLSF:
        return a2nlsf_pool(build, d, family, ref)
    if unit == NLSF2A:
        return nlsf2a_pool(build, d, family)
    if unit == MSVQ:
        return msvq_pool(build, family)
    if unit == BURG:
        return burg_pool(build, sites[0], family)
    return find_lpc_pool(build, family)


_fixtures = {}


def load_cases(build, group):
    """the fixture's cases of a group -> dict family -> (records int32 [n, in_words], reference outputs int32 [n, out_words]); the records are
    regenerated from the family's seed and checked against the fixture's checksum"""
    key = (build.wb, group)
    if key not in _fixtures:
        z = np.load(build.fixture)
        got = {}
        for fam in GROUP_FAMILIES[group]:
            k = "%s/%s" % (group, fam)
            if k + "/out" not in z.files:
                continue
            if k + "/in" in z.files:
                recs = z[k + "/in"].astype(np.int32)
            else:
                recs = np.ascontiguousarray(pool(build, group, fam)[z[k + "/sel"]])
            assert zlib.crc32(recs.tobytes()) == int(z[k + "/crc"]), "the records of %s are not the ones the fixture was made from" % k
            got[fam] = (recs, z[k + "/out"].astype(np.int32))
        _fixtures[key] = got
    return _fixtures[key]


def load_emu_fn(wb):
    """tests/emu's emu_fn of a build"""
    import solo_testlib as T
    lib = T.load_emu_wb() if wb else T.load_emu()
    lib.emu_fn.restype = C.c_int
    lib.emu_fn.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    return lib


def run_emu(build, group, recs, site=None, lib=None):
    """records through emu_fn -> out int32 [n, out_words]"""
    unit, sites, d = build.groups[group]
    lib = lib or load_emu_fn(build.wb)
    iw, ow = build.words(unit)
    recs = np.ascontiguousarray(recs, np.int32)
    assert recs.shape[1] == iw
    out = np.zeros((len(recs), ow), np.int32)
    r = lib.emu_fn(fn_id(unit, sites[0] if site is None else site), len(recs), recs.ctypes.data_as(C.c_void_p), iw, out.ctypes.data_as(C.c_void_p), ow)
    assert r == 0, r
    return out

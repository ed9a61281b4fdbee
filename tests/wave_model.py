"""Plain definitions of the wave-level vocabulary of solo_amd/csrc/solo_wave.h, and the input families its GPU test runs.

Every function takes int arrays of shape (n, 64) -- n independent vectors, one word per lane -- computes in int64 or Python integers
and wraps to 32 bits (64 for wv_sum64) only at its end.  These are the DEFINITIONS the header's comments give (a wrapping sum over the
lanes, a signed maximum, a running sum, the smallest index among the lanes that hold the extreme value ...), not a second
implementation: nothing here knows about rows of 16 lanes except wv_row_sum / wv_col_sum, whose results are defined per row, and
nothing restates a DPP step.  mode0 / mode1 lay the results out in the rows of the probe solo_debug_waveops (solo_api.hip).
mode2 is the workgroup vocabulary (wg_sum, wg_scan_incl, wg_total): four consecutive vectors are the 256 lanes of one workgroup,
vectors beyond the last one count as zeros.

Used by tests/test_gpu_wave_ops.py (GPU, exact equality in every lane) and tests/test_wave_model.py (CPU: the families hold the
cases the GPU test relies on)."""
import functools

import numpy as np

NL = 64
I32_MIN, I32_MAX = -2**31, 2**31 - 1
LANES = np.arange(NL, dtype=np.int64)
# lanes at the edges of the 16-lane rows, of the quads and of the half rows the DPP steps work on
BOUNDARY = (0, 3, 4, 15, 16, 31, 32, 47, 48, 63)

ROWS0 = ("wv_sum", "wv_max", "wv_min", "wv_row_sum", "wv_col_sum", "wv_sum64.lo", "wv_sum64.hi", "wv_scan_incl",
         "wv_argmin(idx=lane).value", "wv_argmin(idx=lane).idx", "wv_argmin(idx=aux).value", "wv_argmin(idx=aux).idx",
         "wv_argmax(idx=lane).value", "wv_argmax(idx=lane).idx", "wv_argmax(idx=aux).value", "wv_argmax(idx=aux).idx",
         "wv_bcast(v, aux[0] & 63)", "wv_bcast(v, aux & 63)", "SX_UNI(wv_max)", "SX_WRLANE/SX_RDLANE samples 0..63",
         "SX_WRLANE/SX_RDLANE samples 64..127", "sx_lcg_first", "sx_lcg_next x1", "sx_lcg_next x2", "sx_lcg_next x3",
         "wv_min(v)", "wv_min(v == vmin ? lane : INT32_MAX)")
_CHAIN = ("a = wv_sum(v)", "b = wv_max(v + a)", "c = wv_min(v ^ b)", "d = wv_sum(c + v)", "e = wv_scan_incl(v + d)",
          "f = wv_argmin(e ^ v, lane).value", "g = wv_argmin(e ^ v, lane).idx", "h = wv_sum64(v * g).lo", "h = wv_sum64(v * g).hi")
ROWS1 = tuple("chain: " + s for s in _CHAIN) + tuple("loop: " + s for s in _CHAIN)
ROWS2 = ("wg_sum", "wg_scan_incl", "wg_total")
WG = 4                                                      # wavefronts (vectors) of a workgroup


def wrap32(x):
    """two's-complement int32 of an int64 array"""
    return ((np.asarray(x, np.int64) + 2**31) % 2**32) - 2**31


def _i64(v):
    v = np.asarray(v)
    assert v.ndim == 2 and v.shape[1] == NL, v.shape
    return v.astype(np.int64)


def _all_lanes(s):
    """a per-vector result, delivered to every lane"""
    return np.repeat(np.asarray(s, np.int64)[:, None], NL, axis=1)


# ---- the definitions ---------------------------------------------------------------------------------------------------------------
def true_sum(v):
    return _i64(v).sum(axis=1)                              # |sum| <= 64 * 2^31: exact in int64


def wv_sum(v):
    return _all_lanes(wrap32(true_sum(v)))


def wv_max(v):
    return _all_lanes(_i64(v).max(axis=1))


def wv_min(v):
    return _all_lanes(_i64(v).min(axis=1))


def wv_row_sum(v):
    """the sum of each 16-lane row, in all lanes of that row"""
    return np.repeat(wrap32(_i64(v).reshape(-1, 4, 16).sum(axis=2)), 16, axis=1)


def wv_col_sum(v):
    """v[j] + v[16 + j] + v[32 + j] + v[48 + j], in lane j of every row"""
    return np.tile(wrap32(_i64(v).reshape(-1, 4, 16).sum(axis=1)), (1, 4))


def true_sum64(lo, hi):
    """per vector, the unwrapped sum (a Python integer) of the 64 signed 64-bit values hi * 2^32 + (lo mod 2^32)"""
    val = _i64(hi).astype(object) * 2**32 + (_i64(lo).astype(object) % 2**32)
    return val.sum(axis=1)


def wv_sum64(lo, hi):
    """(low word, high word) of the sum wrapped to 64 bits, each as int32, in every lane"""
    tot = true_sum64(lo, hi) % 2**64
    return (_all_lanes(wrap32((tot % 2**32).astype(np.int64))), _all_lanes(wrap32((tot // 2**32).astype(np.int64))))


def true_scan(v):
    return np.cumsum(_i64(v), axis=1)


def wv_scan_incl(v):
    return wrap32(true_scan(v))


def _arg(v, idx, best):
    """(extreme value, smallest idx among the lanes that hold it), in every lane"""
    v, idx = _i64(v), _i64(idx)
    bi = np.where(v == best[:, None], idx, np.int64(2**62)).min(axis=1)
    return _all_lanes(best), _all_lanes(bi)


def wv_argmin(v, idx):
    return _arg(v, idx, _i64(v).min(axis=1))


def wv_argmax(v, idx):
    return _arg(v, idx, _i64(v).max(axis=1))


def wv_bcast(v, src):
    """lane l gets the value of lane src[l] (src: (n, 64), already inside 0 .. 63)"""
    return np.take_along_axis(_i64(v), _i64(src), axis=1)


def lane_stream(aux0):
    """the lane-register round trip of the probe: sample i = ((i + 1) * 0x9E3779B1 mod 2^32) ^ aux0 is deposited in lane i & 63 of
    register i >> 6, then sample (i + (aux0 & 63)) & 127 is fetched and deposited at place i; returns the two registers"""
    aux0 = np.asarray(aux0, np.int64)
    i = np.arange(128, dtype=np.int64)[None, :]
    j = (i + (aux0[:, None] & 63)) & 127
    s = wrap32(((j + 1) * 0x9E3779B1) % 2**32 ^ (aux0[:, None] % 2**32))
    return s[:, :64], s[:, 64:]


def lcg_iterates(seed, count):
    """iterates 1 .. count of x -> 907633515 + x * 196314165 (mod 2^32) from `seed`, computed one after the other; (n, count) int32"""
    x = np.asarray(seed, np.int64) % 2**32
    out = np.empty((x.shape[0], count), np.int64)
    for k in range(count):
        x = (907633515 + x * 196314165) % 2**32
        out[:, k] = x
    return wrap32(out)


# ---- the probe's rows ----------------------------------------------------------------------------------------------------------------
def mode0(v, aux):
    """int32 [n][len(ROWS0)][64]: every primitive on the raw inputs"""
    v, aux = _i64(v), _i64(aux)
    aux0 = aux[:, 0]
    lanes = np.broadcast_to(LANES, v.shape)
    rows = [wv_sum(v), wv_max(v), wv_min(v), wv_row_sum(v), wv_col_sum(v)]
    rows += list(wv_sum64(v, aux))
    rows.append(wv_scan_incl(v))
    rows += list(wv_argmin(v, lanes)) + list(wv_argmin(v, aux)) + list(wv_argmax(v, lanes)) + list(wv_argmax(v, aux))
    rows.append(wv_bcast(v, np.broadcast_to((aux0 & 63)[:, None], v.shape)))
    rows.append(wv_bcast(v, aux & 63))
    rows.append(wv_max(v))
    rows += list(lane_stream(aux0))
    it = lcg_iterates(aux0, 4 * NL)                          # lane l of sx_lcg_first: iterate l + 1; each sx_lcg_next: 64 further
    rows += [it[:, k * NL:(k + 1) * NL] for k in range(4)]
    vmin = wv_min(v)
    rows += [vmin, wv_min(np.where(v == vmin, lanes, I32_MAX))]
    assert len(rows) == len(ROWS0)
    return np.stack(rows, axis=1).astype(np.int32)


def _chain(x):
    lanes = np.broadcast_to(LANES, x.shape)
    a = wv_sum(x)
    b = wv_max(wrap32(x + a))
    c = wv_min(x ^ b)
    d = wv_sum(wrap32(c + x))
    e = wv_scan_incl(wrap32(x + d))
    f, g = wv_argmin(e ^ x, lanes)
    p = wrap32(x * g)                                        # the product as an int32, then sign-extended to 64 bits
    h_lo, h_hi = wv_sum64(p, p >> 31)
    return [a, b, c, d, e, f, g, h_lo, h_hi]


def mode1(v, aux):
    """int32 [n][len(ROWS1)][64]: the chain on v, then the results of the last of (aux[0] & 7) + 1 rounds of the same chain, every
    round after the first on x + a + f + g + low word of h (wrapping) of the round before"""
    v, aux = _i64(v), _i64(aux)
    trips = (aux[:, 0] & 7) + 1
    first = _chain(v)
    x, last = v, first
    for t in range(1, 8):
        a, _, _, _, _, f, g, h_lo, _ = last
        nx = wrap32(x + a + f + g + h_lo)
        nxt = _chain(nx)
        go = (t < trips)[:, None]
        x = np.where(go, nx, x)
        last = [np.where(go, n_, l_) for n_, l_ in zip(nxt, last)]
    rows = first + last
    assert len(rows) == len(ROWS1)
    return np.stack(rows, axis=1).astype(np.int32)


def mode2(v):
    """int32 [n][len(ROWS2)][64]: the sum over the workgroup's 256 lanes, the running sum along them, and the scan's total, each
    wrapped to int32; workgroup g holds the vectors 4 g .. 4 g + 3, those at or beyond n being zeros"""
    v = _i64(v)
    n = v.shape[0]
    groups = -(-n // WG)
    flat = np.zeros((groups * WG, NL), np.int64)
    flat[:n] = v
    flat = flat.reshape(groups, WG * NL)
    total = np.repeat(flat.sum(axis=1)[:, None], WG * NL, axis=1)      # |sum| <= 256 * 2^31: exact in int64
    rows = [wrap32(x).reshape(groups * WG, NL)[:n] for x in (total, np.cumsum(flat, axis=1), total)]
    return np.stack(rows, axis=1).astype(np.int32)


# ---- the input families --------------------------------------------------------------------------------------------------------------
def _rand32(rng, shape):
    return rng.integers(I32_MIN, I32_MAX + 1, shape, dtype=np.int64)


def _perms(rng, n):
    return np.stack([rng.permutation(NL) for _ in range(n)]).astype(np.int64)


def _pack(v, aux, tags):
    v, aux = np.asarray(v, np.int64), np.asarray(aux, np.int64)
    assert v.shape == aux.shape == (len(tags), NL)
    assert v.min() >= I32_MIN and v.max() <= I32_MAX and aux.min() >= I32_MIN and aux.max() <= I32_MAX
    return {"v": v.astype(np.int32), "aux": aux.astype(np.int32), "tags": list(tags)}


def family_a():
    """random: full-range int32 in both words (2051 vectors: not a multiple of the 4 waves of a block)"""
    rng = np.random.default_rng(0xA11CE)
    n = 2051
    return _pack(_rand32(rng, (n, NL)), _rand32(rng, (n, NL)), ["random"] * n)


def family_b():
    """extremes and one-hot; each vector twice: aux = a permutation of the lanes, and aux = random words"""
    rng = np.random.default_rng(0xB0B)
    vs, tags = [], []
    for c in (I32_MIN, I32_MAX, -1, 0):
        vs.append(np.full(NL, c, np.int64)); tags.append("all %d" % c)
    for lane in range(NL):
        for val in (1, -1, I32_MIN, I32_MAX):
            x = np.zeros(NL, np.int64); x[lane] = val
            vs.append(x); tags.append("one-hot lane %d value %d" % (lane, val))
        for base, val in ((I32_MAX, I32_MIN), (I32_MAX, 0), (I32_MAX, I32_MAX - 1), (I32_MIN, I32_MAX), (I32_MIN, I32_MIN + 1)):
            x = np.full(NL, base, np.int64); x[lane] = val
            vs.append(x); tags.append("all %d but lane %d value %d" % (base, lane, val))
    v = np.stack(vs)
    n = len(vs)
    return _pack(np.concatenate([v, v]), np.concatenate([_perms(rng, n), _rand32(rng, (n, NL))]),
                 [t + ", aux permutation" for t in tags] + [t + ", aux random" for t in tags])


def family_c():
    """ties: values from {0, 1, 2}; and exactly two lanes at the extreme, for every pair of boundary lanes, as the minimum and as the
    maximum, with idx = lane (the probe's own rows), aux = lane, aux = 63 - lane (the smallest idx is then the HIGHER lane) and
    aux = a random permutation"""
    rng = np.random.default_rng(0xC0FFEE)
    vs, auxs, tags = [], [], []
    n_small = 1024
    small = rng.integers(0, 3, (n_small, NL), dtype=np.int64)
    for k in range(n_small):
        vs.append(small[k])
        auxs.append((63 - LANES) if k % 3 == 0 else (rng.permutation(NL).astype(np.int64) if k % 3 == 1 else _rand32(rng, NL)))
        tags.append("values 0..2")
    for ia, p in enumerate(BOUNDARY):
        for q in BOUNDARY[ia + 1:]:
            for sign, name in ((-1, "min"), (1, "max")):
                for ext in (5000, I32_MAX):                 # (sign * ext: -2^31 + 1 for the minimum; the others stay inside +-1000)
                    for aux, aname in ((LANES.copy(), "lane"), (63 - LANES, "63 - lane"), (rng.permutation(NL).astype(np.int64), "permutation")):
                        x = rng.integers(-1000, 1001, NL, dtype=np.int64)
                        x[p] = x[q] = sign * ext
                        vs.append(x); auxs.append(aux)
                        tags.append("two lanes (%d, %d) at the %s %d, aux = %s" % (p, q, name, sign * ext, aname))
    return _pack(np.stack(vs), np.stack(auxs), tags)


def family_d():
    """64-bit values aux:v: near +-2^31 and +-2^62; low words that sum to exactly 2^32 (two lanes of one row, every pair of places in
    the row; two boundary lanes of different rows); totals beyond 64 bits"""
    rng = np.random.default_rng(0xD00D)
    vals, tags = [], []                                     # Python-integer 64-bit signed values per lane

    def add(x, tag):
        vals.append([int(t) for t in x]); tags.append(tag)

    centres = (2**31, -2**31, 2**62, -2**62, 0, 2**32, -2**32)
    for k in range(512):
        c = rng.integers(0, len(centres), NL)
        add([centres[ci] + int(d) for ci, d in zip(c, rng.integers(-3, 4, NL))], "near +-2^31 / +-2^62")
    for row in range(4):
        for i in range(16):
            for j in range(i + 1, 16):
                x = [0] * NL
                x[16 * row + i], x[16 * row + j] = 0xFFFFFFFF, 1
                add(x, "low words 0xFFFFFFFF + 1 in lanes %d, %d of row %d" % (i, j, row))
        x = [0] * NL
        x[16 * row], x[16 * row + 15] = 2**31, 2**31
        add(x, "low words 2^31 + 2^31 in row %d" % row)
    for ia, p in enumerate(BOUNDARY):
        for q in BOUNDARY[ia + 1:]:
            if p >> 4 != q >> 4:
                for lo_p, lo_q in ((0xFFFFFFFF, 1), (1, 0xFFFFFFFF), (2**31, 2**31)):
                    x = [0] * NL
                    x[p], x[q] = lo_p, lo_q
                    add(x, "low words %#x + %#x in lanes %d, %d of two rows" % (lo_p, lo_q, p, q))
    add([2**26] * NL, "low words 2^26 everywhere")          # 2^30 per row, 2^32 over the wave: only all four rows together carry
    add([2**62] * NL, "all 2^62: the total is 2^68")
    add([-2**63] * NL, "all -2^63")
    add([2**63 - 1] * NL, "all 2^63 - 1")
    for p in (0, 15, 16, 63):
        x = [0] * NL
        x[p], x[63 - p] = -2**63, -2**63
        add(x, "-2^63 twice (lanes %d, %d): the total wraps to 0" % (p, 63 - p))
    for k in range(256):
        add([int(t) for t in rng.integers(-2**63, 2**63 - 1, NL, dtype=np.int64)], "random 64-bit")
    lo = np.array([[((t % 2**32) + 2**31) % 2**32 - 2**31 for t in x] for x in vals], np.int64)
    hi = np.array([[(t % 2**64) // 2**32 for t in x] for x in vals], np.int64)
    return _pack(lo, wrap32(hi), tags)


def family_e():
    """scan: all ones (prefix = lane + 1), one value at each boundary lane, constant extremes, random with wrap"""
    rng = np.random.default_rng(0xE66)
    vs, tags = [np.ones(NL, np.int64)], ["all ones"]
    for c in (I32_MAX, I32_MIN, -1):
        vs.append(np.full(NL, c, np.int64)); tags.append("all %d" % c)
    for lane in BOUNDARY:
        for val in (1, -1, I32_MIN, I32_MAX, 0x12345678):
            x = np.zeros(NL, np.int64); x[lane] = val
            vs.append(x); tags.append("one-hot lane %d value %d" % (lane, val))
    vs.append(LANES + 1); tags.append("ramp")
    n_r = 1024
    vs += list(_rand32(rng, (n_r, NL))); tags += ["random"] * n_r
    v = np.stack(vs)
    return _pack(v, _rand32(rng, v.shape), tags)


FAMILIES = {"A": family_a, "B": family_b, "C": family_c, "D": family_d, "E": family_e}


@functools.lru_cache(maxsize=None)
def family(name):
    """the family's inputs, generated once per process (read-only)"""
    f = FAMILIES[name]()
    f["v"].setflags(write=False); f["aux"].setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def expected(mode, name):
    """the model's rows for a family, computed once per process (read-only)"""
    f = family(name)
    out = (mode0 if mode == 0 else mode1)(f["v"], f["aux"])
    out.setflags(write=False)
    return out

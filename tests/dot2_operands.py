"""Operands and expected values of the packed-pair primitives sx_dot2 / sx_pair (tests/test_gpu_dot2_primitive.py and its CPU half)."""
import functools
import itertools

import numpy as np

HALVES = (-32768, -32767, -1, 0, 1, 32767)
ACCS = (-(1 << 31), -1, 0, 1, (1 << 31) - 1)
N_RANDOM = 1 << 20


def _pack(lo, hi):
    """two int16 halves -> the int32 that holds them (lo in bits 0..15)"""
    return ((np.asarray(lo, np.int64) & 0xFFFF) | ((np.asarray(hi, np.int64) & 0xFFFF) << 16)).astype(np.uint32).view(np.int32)


def _halves(v):
    v = v.view(np.uint32).astype(np.int64)
    lo, hi = v & 0xFFFF, v >> 16
    return lo - ((lo & 0x8000) << 1), hi - ((hi & 0x8000) << 1)


@functools.lru_cache(maxsize=None)
def dot2_operands():
    """every combination of HALVES in the four halves x every accumulator of ACCS, then N_RANDOM seeded random triples (a quarter of
    them with halves drawn from the edges and random accumulators)"""
    e = np.array(list(itertools.product(HALVES, HALVES, HALVES, HALVES, ACCS)), np.int64)
    rng = np.random.default_rng(20261)
    r = rng.integers(-32768, 32768, (N_RANDOM, 4))
    q = N_RANDOM // 4
    r[:q] = np.array(HALVES)[rng.integers(0, len(HALVES), (q, 4))]
    racc = rng.integers(-(1 << 31), 1 << 31, N_RANDOM)
    a = np.concatenate([_pack(e[:, 0], e[:, 1]), _pack(r[:, 0], r[:, 1])])
    b = np.concatenate([_pack(e[:, 2], e[:, 3]), _pack(r[:, 2], r[:, 3])])
    c = np.concatenate([e[:, 4], racc]).astype(np.int32)
    return np.ascontiguousarray(a), np.ascontiguousarray(b), np.ascontiguousarray(c)


def dot2_expected(a, b, c):
    alo, ahi = _halves(a)
    blo, bhi = _halves(b)
    s = c.astype(np.int64) + alo * blo + ahi * bhi                  # exact: |s| < 2^33
    return (s & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


@functools.lru_cache(maxsize=None)
def pair_operands():
    rng = np.random.default_rng(20262)
    n = 4096
    lo = rng.integers(-(1 << 31), 1 << 31, n).astype(np.int32)
    hi = rng.integers(-(1 << 31), 1 << 31, n).astype(np.int32)
    par = (np.arange(n) & 1).astype(np.int32)
    return lo, hi, par


def pair_expected(lo, hi, par):
    """parity 0: the dword `lo` itself; parity 1: its upper half followed by the lower half of `hi`"""
    l, h = lo.view(np.uint32).astype(np.int64), hi.view(np.uint32).astype(np.int64)
    odd = (l >> 16) | ((h & 0xFFFF) << 16)
    return np.where(par == 1, odd, l).astype(np.uint32).view(np.int32)

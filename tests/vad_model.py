"""Independent model of the VAD stage (solo_vad / solo_vad_select, include/solo_mi355x.h) in plain Python integers: the reference's
SKP_Silk_VAD_GetSA_Q8 with its noise-level tracker, the RFC 6464 level of a packet, and the stateful speaker selection.  Written from
the arithmetic the header states and the reference defines; it shares no code with solo_amd/csrc/solo_vad.h."""
import struct
from decimal import ROUND_HALF_EVEN, Decimal, getcontext

import numpy as np

I32_MAX = 0x7FFFFFFF
A_FB1_20 = 5394 << 1
A_FB1_21 = ((20623 << 1) & 0xFFFF) - 0x10000                # the int16 the reference's coefficient wraps to
TILT_WEIGHTS = (30000, 6000, -12000, -12000)
SIGM_SLOPE_Q10 = (237, 153, 73, 30, 12, 7)
SIGM_POS_Q15 = (16384, 23955, 28861, 31213, 32178, 32548)
SIGM_NEG_Q15 = (16384, 8812, 3906, 1554, 589, 219)


def w32(x):
    x &= 0xFFFFFFFF
    return x - 0x100000000 if x & 0x80000000 else x


def s16(x):
    x &= 0xFFFF
    return x - 0x10000 if x & 0x8000 else x


def sat16(x):
    return max(-32768, min(32767, x))


def smulwb(a, b):
    return (a * s16(b)) >> 16


def smlawb(acc, a, b):
    return w32(acc + smulwb(a, b))


def smulww(a, b):
    return w32((a * b) >> 16)


def smulbb(a, b):
    return s16(a) * s16(b)


def div32(a, b):
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def rshift_round(a, s):
    return (a >> 1) + (a & 1) if s == 1 else ((a >> (s - 1)) + 1) >> 1


def add_pos_sat32(a, b):
    s = (a + b) & 0xFFFFFFFF
    return I32_MAX if s & 0x80000000 else s


def clz_frac(x):
    u = x & 0xFFFFFFFF
    lz = 32 - u.bit_length()
    rot = 24 - lz
    if rot > 0:
        r = ((u << (32 - rot)) | (u >> rot)) & 0xFFFFFFFF
    elif rot < 0:
        r = ((u << -rot) | (u >> (32 + rot))) & 0xFFFFFFFF
    else:
        r = u
    return lz, r & 0x7F


def lin2log(x):
    lz, frac = clz_frac(x)
    return ((31 - lz) << 7) + smlawb(frac, frac * (128 - frac), 179)


def sqrt_approx(x):
    if x <= 0:
        return 0
    lz, frac = clz_frac(x)
    y = 32768 if lz & 1 else 46214
    y >>= lz >> 1
    return smlawb(y, y, smulbb(213, frac))


def sigm_q15(x):
    if x < 0:
        x = -x
        if x >= 6 * 32:
            return 0
        return SIGM_NEG_Q15[x >> 5] - smulbb(SIGM_SLOPE_Q10[x >> 5], x & 0x1F)
    if x >= 6 * 32:
        return 32767
    return SIGM_POS_Q15[x >> 5] + smulbb(SIGM_SLOPE_Q10[x >> 5], x & 0x1F)


def filt_bank(x, S):
    """SKP_Silk_ana_filt_bank_1: two first-order all-pass sections -> (low, high), S updated in place"""
    s0, s1 = S
    lo, hi = [], []
    for k in range(len(x) // 2):
        in32 = w32(x[2 * k] << 10)
        Y = w32(in32 - s0)
        X = smlawb(Y, Y, A_FB1_21)
        out_1 = w32(s0 + X)
        s0 = w32(in32 + X)
        in32 = w32(x[2 * k + 1] << 10)
        Y = w32(in32 - s1)
        X = smulwb(Y, A_FB1_20)
        out_2 = w32(s1 + X)
        s1 = w32(in32 + X)
        lo.append(sat16(rshift_round(w32(out_2 + out_1), 11)))
        hi.append(sat16(rshift_round(w32(out_2 - out_1), 11)))
    S[0], S[1] = s0, s1
    return lo, hi


class Vad:
    """one row's state and SKP_Silk_VAD_GetSA_Q8 for frames of 160 or 320 samples"""

    def __init__(self):
        self.ana = [[0, 0], [0, 0], [0, 0]]
        self.xnrg_subfr = [0] * 4
        self.ratio_smth = [100 * 256] * 4
        self.hp = 0
        self.bias = [max(50 // (b + 1), 1) for b in range(4)]
        self.nl = [100 * v for v in self.bias]
        self.inv_nl = [I32_MAX // v for v in self.nl]
        self.counter = 15

    def state_bytes(self):
        words = self.ana[0] + self.ana[1] + self.ana[2] + self.xnrg_subfr + self.ratio_smth
        return np.frombuffer(struct.pack("<14ihxx13i", *(words + [self.hp] + self.nl + self.inv_nl + self.bias + [self.counter])), dtype=np.uint8)

    def noise_levels(self, xnrg):
        min_coef = 32767 // ((self.counter >> 4) + 1) if self.counter < 1000 else 0
        for k in range(4):
            nl = self.nl[k]
            nrg = add_pos_sat32(xnrg[k], self.bias[k])
            inv_nrg = I32_MAX // nrg
            if nrg > w32(nl << 3):
                coef = 1024 >> 3
            elif nrg < nl:
                coef = 1024
            else:
                coef = smulwb(smulww(inv_nrg, nl), 1024 << 1)
            coef = max(coef, min_coef)
            self.inv_nl[k] = smlawb(self.inv_nl[k], inv_nrg - self.inv_nl[k], coef)
            self.nl[k] = min(div32(I32_MAX, self.inv_nl[k]), 0x00FFFFFF)
        self.counter += 1

    def frame(self, x):
        """x: a frame of ints -> (SA_Q8, [SNR_dB_Q7, Tilt_Q15, Quality_Q15[0..3]])"""
        n = len(x)
        assert n in (160, 320)
        X = [None] * 4
        lo, X[3] = filt_bank(x, self.ana[0])
        lo, X[2] = filt_bank(lo, self.ana[1])
        lo, X[1] = filt_bank(lo, self.ana[2])
        h = [v >> 1 for v in lo]
        X[0] = [s16(h[i] - (h[i - 1] if i else self.hp)) for i in range(len(h))]
        self.hp = h[-1]
        xnrg = [0] * 4
        for b in range(4):
            dec = n >> min(4 - b, 3)
            sub = dec >> 2
            e = self.xnrg_subfr[b]
            for s in range(4):
                ss = 0
                for v in X[b][s * sub:(s + 1) * sub]:
                    ss = w32(ss + smulbb(v >> 3, v >> 3))
                e = add_pos_sat32(e, ss if s < 3 else ss >> 1)
            self.xnrg_subfr[b] = ss
            xnrg[b] = e
        self.noise_levels(xnrg)
        sum_sq, tilt = 0, 0
        ratio = [256] * 4
        for b in range(4):
            speech = xnrg[b] - self.nl[b]
            if speech > 0:
                if xnrg[b] & 0xFF800000 == 0:
                    ratio[b] = div32(w32(xnrg[b] << 8), self.nl[b] + 1)
                else:
                    ratio[b] = div32(xnrg[b], (self.nl[b] >> 8) + 1)
                snr = lin2log(ratio[b]) - 8 * 128
                sum_sq = w32(sum_sq + smulbb(snr, snr))
                if speech < 1 << 20:
                    snr = smulwb(w32(sqrt_approx(speech) << 6), snr)
                tilt = smlawb(tilt, TILT_WEIGHTS[b], snr)
        sum_sq = div32(sum_sq, 4)
        snr_db = s16(3 * sqrt_approx(sum_sq))
        sa = sigm_q15(smulwb(45000, snr_db) - 128)
        tilt_q15 = w32((sigm_q15(tilt) - 16384) << 1)
        speech = 0
        for b in range(4):
            speech = w32(speech + (b + 1) * ((xnrg[b] - self.nl[b]) >> 4))
        if speech <= 0:
            sa >>= 1
        elif speech < 32768:
            speech = sqrt_approx(w32(speech << 15))
            sa = smulwb(32768 + speech, sa)
        sa_q8 = min(sa >> 7, 255)
        smooth = s16(smulwb(4096, smulwb(sa, sa)))
        quality = []
        for b in range(4):
            self.ratio_smth[b] = smlawb(self.ratio_smth[b], ratio[b] - self.ratio_smth[b], smooth)
            snr = 3 * (lin2log(self.ratio_smth[b]) - 8 * 128)
            quality.append(sigm_q15((snr - 16 * 128) >> 4))
        return sa_q8, [snr_db, tilt_q15] + quality

    def packet(self, x, frame):
        """x: int16 array of a packet -> (sa uint8 [F], detail int32 [F, 6])"""
        v = [int(s) for s in x]
        out = [self.frame(v[f:f + frame]) for f in range(0, len(v), frame)]
        return np.array([o[0] for o in out], dtype=np.uint8), np.array([o[1] for o in out], dtype=np.int32)


# ---- the RFC 6464 level ------------------------------------------------------------------------------------------------------------------
_T = None


def thresholds():
    """T_k = round(2^50 * 10^(-k / 10)), k = 0 .. 127"""
    global _T
    if _T is None:
        getcontext().prec = 80
        _T = [int((Decimal(2) ** 50 * Decimal(10) ** (Decimal(-k) / 10)).quantize(Decimal(1), rounding=ROUND_HALF_EVEN)) for k in range(128)]
    return _T


def level_of_energy(E, packet_samples):
    for k, t in enumerate(thresholds()):
        if (E << 20) >= packet_samples * t:
            return k
    return 127


def level(x):
    """x: int16 array of a packet -> its level in -dBov"""
    v = x.astype(np.int64)
    return level_of_energy(int((v * v).sum()), v.size)


# ---- the selection ---------------------------------------------------------------------------------------------------------------------------
class Select:
    """state (talking, hang, picked) of n_rows rows; run() walks the packets of a call"""

    def __init__(self, n_rows):
        self.t = [0] * n_rows
        self.h = [0] * n_rows
        self.s = [0] * n_rows

    def state_words(self):
        return np.array([self.t, self.h, self.s, [0] * len(self.t)], dtype=np.int32).T.copy()

    def run(self, sa, level, room, n_rooms, max_speakers=3, on=128, off=64, hang=5, stick=6, gain=None, rows=None):
        """sa [n, P, F], level [n, P], room [n] -> dict(sel uint8 [n, P], gain_out int16 [n], keep uint8 [n], dominant int32 [n_rooms, P],
        count dict); entries of rows outside every room hold the fill values 0x5A (sel, keep) and 0x5A5A (gain_out)"""
        n, P, _ = sa.shape
        rows = list(range(n)) if rows is None else [int(r) for r in rows]
        sel = np.full((n, P), 0x5A, dtype=np.uint8)
        gain_out = np.full(n, 0x5A5A, dtype=np.int16)
        keep = np.full(n, 0x5A, dtype=np.uint8)
        dominant = np.full((n_rooms, P), -1, dtype=np.int32)
        members = [[i for i in range(n) if room[i] == r] for r in range(n_rooms)]
        selected = changes = 0
        cand = {}
        for p in range(P):
            for r_id, mem in enumerate(members):
                keys = []
                for i in mem:
                    r = rows[i]
                    a = int(sa[i, p].max())
                    if a >= (off if self.t[r] else on):
                        self.t[r], self.h[r], cand[i] = 1, hang, True
                    else:
                        self.t[r], cand[i], self.h[r] = 0, self.h[r] > 0, max(self.h[r] - 1, 0)
                    if cand[i]:
                        keys.append((-((127 - min(int(level[i, p]), 127)) + (stick if self.s[r] else 0)), -self.s[r], i))
                keys.sort()
                chosen = [k[2] for k in keys[:max_speakers]]
                for i in mem:
                    s = 1 if i in chosen else 0
                    changes += s != self.s[rows[i]]
                    selected += s
                    self.s[rows[i]] = s
                    sel[i, p] = s
                if chosen:
                    dominant[r_id, p] = chosen[0]
        for mem in members:
            for i in mem:
                g = 4096 if gain is None else max(int(gain[i]), 0)
                gain_out[i] = g if self.s[rows[i]] else 0
                keep[i] = 1 if cand[i] else 0
        count = dict(rows=sum(len(m) for m in members), rooms=sum(1 for m in members if m), selected=selected, changes=changes)
        return dict(sel=sel, gain_out=gain_out, keep=keep, dominant=dominant, count=count)

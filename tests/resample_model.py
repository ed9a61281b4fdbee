"""Independent statement of the reference's resampler (SKP_Silk_resampler_init / SKP_Silk_resampler of the fixed-point tree) for the
conversions solo_resample offers: plain Python integers, one sample at a time, written from the reference's arithmetic and sharing
no code with solo_amd/csrc/solo_resample.h.  The coefficient values are parsed out of the generated table file.

    m = Model(fs_in, fs_out)            # state zeroed
    out = m.run(int16 samples)          # any whole number of 10 ms batches; the state carries over
    m.state_bytes()                     # the 96 bytes sIIR[6] | sFIR[16] | sDown2[2]
    Model.from_state(fs_in, fs_out, b)  # continue from 96 recorded bytes
"""
import os
import re

import numpy as np

_INC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "solo_amd", "csrc", "solo_resample_tables.inc")


def _tables():
    text = re.sub(r"/\*.*?\*/", "", open(_INC).read(), flags=re.S)
    return {m.group(1): [int(v) for v in m.group(2).replace("\n", " ").split(",") if v.strip()]
            for m in re.finditer(r"T_(\w+)\[\d+\]\s*=\s*\{([^}]*)\}", text)}


TAB = _tables()


def w32(x):
    """wrap to a signed 32-bit value"""
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x & 0x80000000 else x


def s16(x):
    x &= 0xFFFF
    return x - 65536 if x & 0x8000 else x


def smulwb(a, b):
    return w32((a * s16(b)) >> 16)


def smlawb(acc, a, b):
    return w32(acc + smulwb(a, b))


def sat16(x):
    return 32767 if x > 32767 else (-32768 if x < -32768 else x)


def rshift_round(a, s):
    return w32((a >> 1) + (a & 1)) if s == 1 else (w32((a >> (s - 1)) + 1) >> 1)


def supported(fs_in, fs_out):
    rates = (8000, 16000, 32000, 48000)
    return fs_in in rates and fs_out in rates and (fs_out * 3 == fs_in or fs_out * 3 == fs_in * 2 or fs_out * 2 == fs_in or
                                                   fs_out == fs_in * 2 or fs_out == fs_in * 3 or fs_out * 2 == fs_in * 3)


class Model:
    def __init__(self, fs_in, fs_out):
        assert supported(fs_in, fs_out)
        self.fs_in, self.fs_out = fs_in, fs_out
        self.batch = fs_in // 100
        self.iir = [0] * 6
        self.fir = [0] * 16
        self.down2 = [0, 0]
        self.up2 = 0
        if fs_out < fs_in:
            self.path = "down"
            if fs_out * 3 == fs_in:
                self.coefs, self.fracs = TAB["rs_down_1_3"], 1
            elif fs_out * 3 == fs_in * 2:
                self.coefs, self.fracs = TAB["rs_down_2_3"], 2
            else:
                self.coefs, self.fracs = TAB["rs_down_1_2"], 1
        elif fs_out == 2 * fs_in:
            self.path = "up2"
        else:
            self.path, self.up2 = "iir_fir", 1
            self.hq = fs_in <= 24000
        inv = ((fs_in << (14 + self.up2)) // fs_out) << 2
        while w32((inv * fs_out) >> 16) < (fs_in << self.up2):
            inv += 1
        self.inv = inv

    @classmethod
    def from_state(cls, fs_in, fs_out, state):
        m = cls(fs_in, fs_out)
        w = np.frombuffer(bytes(bytearray(state)), dtype="<i4")
        m.iir, m.fir, m.down2 = [int(v) for v in w[0:6]], [int(v) for v in w[6:22]], [int(v) for v in w[22:24]]
        return m

    def state_bytes(self):
        return np.array(self.iir + self.fir + self.down2, dtype="<i4").view(np.uint8).copy()

    # ---- the serial parts ----
    def _ar2(self, x):
        S, A = self.iir, self.coefs
        out = []
        for v in x:
            o = w32(S[0] + (v << 8))
            out.append(o)
            o = w32(o << 2)
            S[0] = smlawb(S[1], o, A[0])
            S[1] = smulwb(o, A[1])
        return out

    def _up2_hq(self, x):
        S = self.iir
        h0, h1, nt = TAB["rs_up2_hq_0"], TAB["rs_up2_hq_1"], TAB["rs_up2_hq_notch"]
        out = []
        for v in x:
            in32 = v << 10
            Y = w32(in32 - S[0]); X = smulwb(Y, h0[0]); o1 = w32(S[0] + X); S[0] = w32(in32 + X)
            Y = w32(o1 - S[1]); X = smlawb(Y, Y, h0[1]); o2 = w32(S[1] + X); S[1] = w32(o1 + X)
            o2 = smlawb(o2, S[5], nt[2]); o2 = smlawb(o2, S[4], nt[1]); o1 = smlawb(o2, S[4], nt[0]); S[5] = w32(o2 - S[5])
            out.append(sat16(smlawb(256, o1, nt[3]) >> 9))
            Y = w32(in32 - S[2]); X = smulwb(Y, h1[0]); o1 = w32(S[2] + X); S[2] = w32(in32 + X)
            Y = w32(o1 - S[3]); X = smlawb(Y, Y, h1[1]); o2 = w32(S[3] + X); S[3] = w32(o1 + X)
            o2 = smlawb(o2, S[4], nt[2]); o2 = smlawb(o2, S[5], nt[1]); o1 = smlawb(o2, S[5], nt[0]); S[4] = w32(o2 - S[4])
            out.append(sat16(smlawb(256, o1, nt[3]) >> 9))
        return out

    def _up2_lq(self, x):
        S, lq = self.iir, TAB["rs_up2_lq"]
        out = []
        for v in x:
            in32 = v << 10
            Y = w32(in32 - S[0]); X = smulwb(Y, lq[0]); o = w32(S[0] + X); S[0] = w32(in32 + X)
            out.append(sat16(rshift_round(o, 10)))
            Y = w32(in32 - S[1]); X = smlawb(Y, Y, lq[1]); o = w32(S[1] + X); S[1] = w32(in32 + X)
            out.append(sat16(rshift_round(o, 10)))
        return out

    # ---- one batch of 10 ms ----
    def _down_batch(self, x):
        buf = self.fir[:12] + self._ar2(x)
        n, f, out = len(x), self.coefs[2:], []
        idx = 0
        while idx < (n << 16):
            b = buf[idx >> 16: (idx >> 16) + 12]
            if self.fracs == 1:
                r = smulwb(w32(b[0] + b[11]), f[0])
                for t in range(1, 6):
                    r = smlawb(r, w32(b[t] + b[11 - t]), f[t])
            else:
                ind = smulwb(idx & 0xFFFF, self.fracs)
                p = f[6 * ind: 6 * ind + 6]
                r = smulwb(b[0], p[0])
                for t in range(1, 6):
                    r = smlawb(r, b[t], p[t])
                p = f[6 * (self.fracs - 1 - ind): 6 * (self.fracs - 1 - ind) + 6]
                for t in range(6):
                    r = smlawb(r, b[11 - t], p[t])
            out.append(sat16(rshift_round(r, 6)))
            idx += self.inv
        self.fir[:12] = buf[n: n + 12]
        return out

    def _hist16(self):
        """the six int16 of history that sFIR[0..3) holds"""
        return [s16(self.fir[i >> 1] >> (16 * (i & 1))) for i in range(6)]

    def _iir_fir_batch(self, x):
        up = self._up2_hq(x) if self.hq else self._up2_lq(x)
        buf = self._hist16() + up
        n2, tab, out = 2 * len(x), TAB["rs_frac144"], []
        idx = 0
        while idx < (n2 << 16):
            ti = smulwb(idx & 0xFFFF, 144)
            b = buf[idx >> 16: (idx >> 16) + 6]
            f0, f1 = tab[3 * ti: 3 * ti + 3], tab[3 * (143 - ti): 3 * (143 - ti) + 3]
            r = b[0] * f0[0] + b[1] * f0[1] + b[2] * f0[2] + b[3] * f1[2] + b[4] * f1[1] + b[5] * f1[0]
            out.append(sat16(rshift_round(w32(r), 15)))
            idx += self.inv
        h = buf[n2: n2 + 6]
        for i in range(3):
            self.fir[i] = w32((h[2 * i] & 0xFFFF) | ((h[2 * i + 1] & 0xFFFF) << 16))
        return out

    def run(self, x):
        x = [int(v) for v in np.asarray(x).reshape(-1)]
        assert len(x) % self.batch == 0
        out = []
        for b0 in range(0, len(x), self.batch):
            xb = x[b0: b0 + self.batch]
            out += self._down_batch(xb) if self.path == "down" else (self._up2_hq(xb) if self.path == "up2" else self._iir_fir_batch(xb))
        return np.array(out, dtype=np.int16)


def run_rows(fs_in, fs_out, pcm, states=None):
    """pcm int16 [n, P, L] (one call) -> (out int16 [n, P, L'], state uint8 [n, 96]); states: uint8 [n, 96] to continue from, or None"""
    n, P, L = pcm.shape
    outs, sts = [], []
    for i in range(n):
        m = Model(fs_in, fs_out) if states is None else Model.from_state(fs_in, fs_out, states[i])
        outs.append(m.run(pcm[i]).reshape(P, -1))
        sts.append(m.state_bytes())
    return np.stack(outs), np.stack(sts)

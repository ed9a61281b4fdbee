"""Input families of tests/test_gpu_burg_sites.py (and of its CPU companion and fixture generator): each is chosen to reach one branch
of sx_burg_modified's recursion.  64 streams x 6 packets each, every stream of a family different; deterministic."""
import numpy as np

N, P = 64, 6
RATE, RATE_WB = 13600, 24000
SLOT = 512
FAMILIES = ("silence", "lsb_noise", "white_full_scale", "square_full_scale", "speech_like", "sinusoid", "two_tone", "silence_then_full_scale", "nyquist_full_scale")
WB = "speech_like_32k"            # the 32 kHz build: its order-16 analysis keeps the LDS form of the recursion


def _i16(x):
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def family(name):
    """-> int16 [N, P, 640] (1280 for the 32 kHz family)"""
    n = P * 640
    t = np.arange(n) / 16000.0
    rng = np.random.default_rng(sum(name.encode()) + 20260)
    if name == "silence":                       # digital silence; stream i > 0 carries i isolated LSBs so that the streams differ
        x = np.zeros((N, n), np.int16)
        for i in range(1, N):
            x[i, rng.integers(0, n, i)] = 1
    elif name == "lsb_noise":                   # +-1 LSB: rshifts <= -2, the hi = false recursion
        x = rng.integers(-1, 2, (N, n)).astype(np.int16)
    elif name == "white_full_scale":            # rshifts at and above MAX_RSHIFTS
        x = rng.integers(-32768, 32768, (N, n)).astype(np.int16)
    elif name == "square_full_scale":
        x = np.stack([_i16(32767 * np.sign(np.sin(2 * np.pi * (70.0 + 37.0 * i) * t + 0.1))) for i in range(N)])
    elif name == "speech_like":                 # the usual regime
        from solo_amd.synth import synth_stream
        x = np.stack([synth_stream(7100 + i, P).reshape(-1) for i in range(N)])
    elif name == "sinusoid":                    # - 6 dBFS, near-singular: the |num| >= den exit
        x = np.stack([_i16(16384 * np.sin(2 * np.pi * (110.0 + 53.0 * i) * t)) for i in range(N)])
    elif name == "two_tone":                    # - 6 dBFS peak
        x = np.stack([_i16(8192 * (np.sin(2 * np.pi * (200.0 + 31.0 * i) * t) + np.sin(2 * np.pi * (1900.0 + 17.0 * i) * t + 1.0))) for i in range(N)])
    elif name == "silence_then_full_scale":     # the two runs of a frame in different regimes.  Even streams: from the third packet's first
        x = rng.integers(-32768, 32768, (N, n)).astype(np.int16)     # sample; odd streams: from up to 630 samples into it
        for i in range(N):
            x[i, :2 * 640 + (i % 2) * 10 * (i // 2 + 1)] = 0
    elif name == "nyquist_full_scale":          # +A, -A, +A ...: all of it in the high band, whose recursion leaves through the exit
        x = np.stack([_i16((32767 - 200 * i) * (1.0 - 2.0 * (np.arange(n) % 2))) for i in range(N)])
    elif name == WB:
        from solo_amd.synth import synth_stream
        return np.stack([synth_stream(7300 + i, 2 * P).reshape(P, 1280) for i in range(N)])
    else:
        raise KeyError(name)
    return np.ascontiguousarray(x.reshape(N, P, 640))


def ctor(name):
    """arguments of RefEncoder / SoloBatch for a family"""
    return dict(rate=RATE_WB, samplerate=32000) if name == WB else dict(rate=RATE)


def reference(name):
    """the compiled reference over a family -> (bits uint8 [N, P, SLOT], nbytes int16 [N, P, 2]); every packet must encode (a returned
    length equal to nBytes0 and positive)"""
    import refcodec as R
    pcm = family(name)
    bits, nb = np.zeros((N, P, SLOT), np.uint8), np.zeros((N, P, 2), np.int16)
    for i in range(N):
        e = R.RefEncoder("fix", **ctor(name))
        for p in range(P):
            pl, n0, n1 = e.encode(pcm[i, p])
            assert 0 < len(pl) == n0 <= SLOT and 0 <= n1 <= n0, (name, i, p, len(pl), n0, n1)
            bits[i, p, :n0] = np.frombuffer(pl, np.uint8)
            nb[i, p] = (n0, n1)
        e.close()
    return bits, nb

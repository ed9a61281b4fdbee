"""Input families of tests/test_gpu_dot_sites.py (and of its CPU companion and fixture generator): signals for the sites that sum products
of 16-bit samples two at a time (sx_dot2, solo_fix.h) -- the two pitch stages, the whitening and residual filters, the first row of the Burg
correlations.  64 streams x 6 packets each, every stream of a family different; deterministic."""
import numpy as np

N, P = 64, 6
RATE, RATE_WB = 13600, 24000
SLOT = 512
FAMILIES = ("silence", "lsb_noise", "white_full_scale", "square_full_scale", "alternating_full_scale", "speech_like", "voiced_harmonic",
            "silence_then_full_scale")
WB = "voiced_harmonic_32k"        # the 32 kHz build: order-16 filters, 16 -> 8 kHz decimation in front of the same two pitch stages


def _i16(x):
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def _harmonic(period, n, fs_ratio, rng):
    """a pulse-like voiced signal: harmonics of 16000 * fs_ratio / period Hz falling off as 1 / h up to 3.4 kHz, - 9 dBFS peak, over a
    noise floor 50 dB down"""
    t = np.arange(n, dtype=np.float64)
    H = max(1, int(period * 3400.0 / (16000.0 * fs_ratio)))
    x = sum(np.sin(2 * np.pi * h * t / period + 0.3 * h) / h for h in range(1, H + 1))
    return 11000.0 * x / np.abs(x).max() + rng.normal(0.0, 30.0, n)


def family(name):
    """-> int16 [N, P, 640] (1280 for the 32 kHz family)"""
    n = P * 640
    t = np.arange(n) / 16000.0
    rng = np.random.default_rng(sum(name.encode()) + 20270)
    if name == "silence":                       # digital silence; stream i > 0 carries i isolated LSBs so that the streams differ
        x = np.zeros((N, n), np.int16)
        for i in range(1, N):
            x[i, rng.integers(0, n, i)] = 1
    elif name == "lsb_noise":
        x = rng.integers(-1, 2, (N, n)).astype(np.int16)
    elif name == "white_full_scale":
        x = rng.integers(-32768, 32768, (N, n)).astype(np.int16)
    elif name == "square_full_scale":           # runs of -32768 / +32767: pair sums at the 2^31 edge, scaling shifts > 0
        x = np.stack([np.where(np.sin(2 * np.pi * (60.0 + 29.0 * i) * t + 0.1) >= 0, 32767, -32768).astype(np.int16) for i in range(N)])
    elif name == "alternating_full_scale":      # +A, -A, ...: the sign flips every 1 .. 4 samples (stream i: 1 + i % 4), A = 32767 - 150 i, and
        # every 97th sample is -32768
        x = np.stack([_i16((32767 - 150 * i) * (1.0 - 2.0 * ((np.arange(n) // (1 + (i % 4))) % 2))) for i in range(N)])
        x[:, 0::97] = -32768
    elif name == "speech_like":                 # the benchmark's generator
        from solo_amd.synth import synth_stream
        x = np.stack([synth_stream(7500 + i, P).reshape(-1) for i in range(N)])
    elif name == "voiced_harmonic":             # periods of 41 .. 230 samples at 16 kHz: 8 kHz lags 20 .. 115 of both parities
        x = np.stack([_i16(_harmonic(41 + 3 * i, n, 1.0, rng)) for i in range(N)])
    elif name == "silence_then_full_scale":     # the onset 9 * i samples into the third packet: even and odd offsets
        x = rng.integers(-32768, 32768, (N, n)).astype(np.int16)
        for i in range(N):
            x[i, :2 * 640 + 9 * i] = 0
    elif name == WB:
        rng = np.random.default_rng(20271)
        return np.stack([_i16(_harmonic(82 + 6 * i + (i % 2), 2 * n, 2.0, rng)).reshape(P, 1280) for i in range(N)])
    else:
        raise KeyError(name)
    return np.ascontiguousarray(x.reshape(N, P, 640))


def ctor(name):
    """arguments of RefEncoder / SoloBatch for a family"""
    return dict(rate=RATE_WB, samplerate=32000) if name == WB else dict(rate=RATE)


def reference(name):
    """the compiled reference over a family -> (bits uint8 [N, P, SLOT], nbytes int16 [N, P, 2]); every packet must encode (a returned
    length equal to nBytes0, positive and within the slot)"""
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

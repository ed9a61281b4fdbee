"""Independent model of solo_mix (include/solo_mi355x.h), written from the rules of the interface, not from solo_amd/csrc/solo_mix.h:
int64 numpy arithmetic and Python sorting, room by room and packet by packet."""
import numpy as np


def model_mix(pcm, room, n_rooms, gain=None, max_speakers=0, out=None, energy=None, mixed=None):
    """pcm int16 [n, P, L], room int [n], gain int16 [n] or None -> dict(out, energy, mixed, count); out / energy / mixed start from the
    given arrays (copied), so rows the call must not write keep their fill.  A room id outside [-1, n_rooms): count rows = -1, nothing
    else changes."""
    n, P, L = pcm.shape
    room = np.asarray(room).astype(np.int64)
    out = np.zeros((n, P, L), np.int16) if out is None else out.copy()
    energy = np.zeros((n, P), np.int64) if energy is None else energy.copy()
    mixed = np.zeros((n, P), np.uint8) if mixed is None else mixed.copy()
    if ((room < -1) | (room >= n_rooms)).any():
        return dict(out=out, energy=energy, mixed=mixed, count=dict(rows=-1, rooms=None, clipped=None))
    g = np.full(n, 4096, np.int64) if gain is None else np.maximum(np.asarray(gain).astype(np.int64), 0)
    clipped = 0
    ids = [int(r) for r in np.unique(room) if r >= 0]
    for r in ids:
        M = np.flatnonzero(room == r)
        c = (pcm[M].astype(np.int64) * g[M][:, None, None] + 2048) >> 12         # [m, P, L]
        e = (c * c).sum(axis=2)                                                  # [m, P]
        energy[M] = e
        for p in range(P):
            if max_speakers <= 0 or max_speakers >= len(M):
                sel = list(range(len(M)))
            else:
                order = sorted(range(len(M)), key=lambda k: (-int(e[k, p]), int(M[k])))
                sel = order[:max_speakers]
            flag = np.zeros(len(M), bool)
            flag[sel] = True
            S = c[sel, p].sum(axis=0)
            o = S[None, :] - np.where(flag[:, None], c[:, p], 0)
            clipped += int(((o > 32767) | (o < -32768)).sum())
            out[M, p] = np.clip(o, -32768, 32767).astype(np.int16)
            mixed[M, p] = flag
    return dict(out=out, energy=energy, mixed=mixed, count=dict(rows=int((room >= 0).sum()), rooms=len(ids), clipped=clipped))


ROOM_SIZES = (1, 2, 3, 64, 65, 1000, 4, 5, 8, 9, 16, 17, 2, 2, 6)
GAINS = (0, -5, 4096, 32767)


def mix_case(seed, P, L, sizes=ROOM_SIZES, loose=20):
    """A conference floor with everything the interface names: rooms of `sizes` members scattered over the rows, `loose` rows in no room,
    gains 0 / negative / 4096 / 32767 / random, full-scale rows, and identical loud rows inside rooms (energy ties that the row index
    must decide).  -> (pcm int16 [n, P, L], room int32 [n], gain int16 [n], n_rooms)"""
    rng = np.random.default_rng(seed)
    n = sum(sizes) + loose
    room = np.full(n, -1, np.int32)
    rows = rng.permutation(n)
    # room ids are not dense: every other id stays empty
    k = 0
    for r, m in enumerate(sizes):
        room[rows[k:k + m]] = 2 * r
        k += m
    n_rooms = 2 * len(sizes) + 3
    level = rng.integers(0, 12, (n, P, 1))
    pcm = (rng.integers(-32768, 32768, (n, P, L)) >> level).astype(np.int16)
    gain = rng.integers(0, 8192, n).astype(np.int16)
    q = min(40, n // 4)
    gain[rng.permutation(n)[:4 * q].reshape(4, q)] = np.array(GAINS, np.int16)[:, None]
    for r, m in enumerate(sizes):
        M = np.flatnonzero(room == 2 * r)
        if m >= 2:                               # full scale, one sign: the sums saturate
            pcm[M[0]] = 32767
            pcm[M[1]] = -32768 if m > 2 else 32767
            gain[M[:2]] = 32767 if r % 2 else 4096
        if m >= 3:                               # identical loud rows: the loudest of the room in every packet, tied
            twins = M[-min(5, m - 1):]
            pcm[twins] = (rng.integers(-32768, 32768, (1, P, L)) | 0x4000).astype(np.int16)
            gain[twins] = 32767
        if m >= 60:                              # two silent rows: tied at the quiet end
            pcm[M[2:4]] = 0
    return pcm, room, gain, n_rooms


def ties_decide(energy, room, max_speakers):
    """(room, packet) pairs where the last chosen and the first rejected member have the same energy"""
    hits = 0
    for r in np.unique(room[room >= 0]):
        M = np.flatnonzero(room == r)
        if 0 < max_speakers < len(M):
            e = -np.sort(-energy[M], axis=0)
            hits += int((e[max_speakers - 1] == e[max_speakers]).sum())
    return hits

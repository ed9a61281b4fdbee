"""Independent model of solo_mix_selected (include/solo_mi355x.h), written from the rules of the interface, not from
solo_amd/csrc/solo_mix_selected.h: numpy and plain Python loops, room by room and packet by packet.  Nothing here calls the library, the
host form or the models of the other mixing calls."""
import numpy as np

MAX_SELECTED = 64


def model_mix_selected(pcm, room, n_rooms, sel, gain=None, keep=None, slots=None, fill=None):
    """pcm int16 [n, P, L], room int [n], sel uint8 [n, P], gain int16 [n] / keep uint8 [n] / slots int [n] or None -> dict(pcm_spk [n,P,L],
    spk_list [n], spk_rows [n], pcm_room [n_rooms,P,L], room_list [n_rooms], source [n], room_nsel [n_rooms,P], energy [n,P], count).
    fill: dict of arrays the outputs start from (copied), so what the call must not write keeps its fill.  A device refusal (a room id
    outside [-1, n_rooms), slots that do not grow strictly from a non-negative start, more than 64 selected rows in a (room, packet)):
    count rows = -1, nothing else changes."""
    n, P, L = pcm.shape
    room = np.asarray(room).astype(np.int64)
    sel = np.asarray(sel)
    assert sel.shape == (n, P)
    fill = fill or {}
    start = lambda k, shape, dt: np.zeros(shape, dt) if k not in fill else fill[k].copy()
    w = dict(pcm_spk=start("pcm_spk", (n, P, L), np.int16), spk_list=start("spk_list", (n,), np.int32), spk_rows=start("spk_rows", (n,), np.int32),
             pcm_room=start("pcm_room", (n_rooms, P, L), np.int16), room_list=start("room_list", (n_rooms,), np.int32),
             source=start("source", (n,), np.int32), room_nsel=start("room_nsel", (n_rooms, P), np.uint8), energy=start("energy", (n, P), np.int64))
    refused = dict(rows=-1, rooms=None, speakers=None, shared=None, clipped=None, selected=None, silent=None)
    bad = bool(((room < -1) | (room >= n_rooms)).any())
    if slots is not None:
        s = np.asarray(slots).astype(np.int64)
        bad |= bool(s[0] < 0 or (np.diff(s) <= 0).any())
    if bad:
        w["count"] = refused
        return w
    member = room >= 0
    on = (sel != 0) & member[:, None]                                           # [n, P]: a row in no room is never selected
    for r in range(n_rooms):
        if (on[room == r].sum(axis=0) > MAX_SELECTED).any():
            w["count"] = refused
            return w
    g = np.full(n, 4096, np.int64) if gain is None else np.maximum(np.asarray(gain).astype(np.int64), 0)
    c = (pcm.astype(np.int64) * g[:, None, None] + 2048) >> 12                  # [n, P, L]
    w["energy"][member] = (c[member] * c[member]).sum(axis=2)
    kept = np.zeros(n, bool) if keep is None else np.asarray(keep) != 0
    spk = member & (on.any(axis=1) | kept)
    S = np.zeros((n_rooms, P, L), np.int64)
    nsel = np.zeros((n_rooms, P), np.int64)
    for r in range(n_rooms):
        for p in range(P):
            for i in np.flatnonzero((room == r) & on[:, p]):
                S[r, p] += c[i, p]
                nsel[r, p] += 1
    clipped = 0
    rows = np.flatnonzero(spk)
    for k, i in enumerate(rows):
        o = S[room[i]] - np.where(on[i][:, None], c[i], 0)
        clipped += int(((o > 32767) | (o < -32768)).sum())
        w["pcm_spk"][k] = np.clip(o, -32768, 32767)
        w["spk_rows"][k] = i
        w["spk_list"][k] = i if slots is None else slots[i]
        w["source"][i] = k
    shared = [r for r in range(n_rooms) if (member & ~spk & (room == r)).any()]
    silent = 0
    for j, r in enumerate(shared):
        clipped += int(((S[r] > 32767) | (S[r] < -32768)).sum())
        w["pcm_room"][j] = np.clip(S[r], -32768, 32767)
        w["room_list"][j] = r
        w["room_nsel"][j] = nsel[r]
        w["source"][member & ~spk & (room == r)] = n + j
        silent += int((nsel[r] == 0).sum())
    w["source"][~member] = -1
    w["count"] = dict(rows=int(member.sum()), rooms=len(set(room[member].tolist())), speakers=len(rows), shared=len(shared), clipped=clipped,
                      selected=int(on.sum()), silent=silent)
    return w


def heard(w, n):
    """what every row of the call hears: [n, P, L] picked out of the two tables through source (zeros for a row in no room)"""
    out = np.zeros((n,) + w["pcm_spk"].shape[1:], np.int16)
    for i in range(n):
        s = int(w["source"][i])
        if s >= n:
            out[i] = w["pcm_room"][s - n]
        elif s >= 0:
            out[i] = w["pcm_spk"][s]
    return out


SIZES = dict(one=1, nobody=2, moving=5, everyone=6, some=9, big=70, kept=4, steady=3)


def selected_case(seed, P, L, big=70, loose=6):
    """A floor with everything the interface of solo_mix_selected names.  Rooms (ids 0, 2, 4, ...: every other id stays empty), scattered
    over the rows:
      one       1 member, selected in every packet (all of the room: not shared)
      nobody    2 members, none ever selected, none kept (shared, every packet silent)
      moving    5 members, member p % 5 alone in packet p
      everyone  6 members, all selected in every packet (not shared); two full-scale rows of one sign, so every output saturates
      some      9 members: three loud ones in packet 0 (S saturates), one of them in packet 1, none in packet 2; a kept row that is never
                selected; sel bytes other than 1
      big       `big` members: min(big, 64) selected in packet 0, 5 in packet 1, 1 in packet 2; among the selected a gain of 0, a negative
                gain and 32767; a kept row that is never selected
      kept      4 members, none selected, all kept: speakers without a room row, who hear zeros
      steady    3 members, the same one in every packet
    `loose` rows in no room, two of them with sel set and one kept; slots with gaps.
    -> (pcm int16 [n,P,L], room int32 [n], gain int16 [n], n_rooms, sel uint8 [n,P], keep uint8 [n], slots int32 [n], marks: room name ->
    its member rows in increasing order, and `loose`)"""
    rng = np.random.default_rng(seed)
    sizes = dict(SIZES, big=big)
    n = sum(sizes.values()) + loose
    room = np.full(n, -1, np.int32)
    order = rng.permutation(n)
    marks, k = {}, 0
    for r, (name, m) in enumerate(sizes.items()):
        room[order[k:k + m]] = 2 * r
        marks[name] = np.sort(order[k:k + m])
        k += m
    marks["loose"] = np.sort(order[k:])
    n_rooms = 2 * len(sizes) + 3
    level = rng.integers(0, 12, (n, P, 1))
    pcm = (rng.integers(-32768, 32768, (n, P, L)) >> level).astype(np.int16)
    gain = rng.integers(1, 8192, n).astype(np.int16)
    sel = np.zeros((n, P), np.uint8)
    keep = np.zeros(n, np.uint8)
    sel[marks["one"]] = 1
    for p in range(P):
        sel[marks["moving"][p % 5], p] = 1
    ev = marks["everyone"]
    sel[ev] = 1
    pcm[ev[:2]] = 32767
    gain[ev[:2]] = 4096
    so = marks["some"]
    pcm[so[:3]] = (rng.integers(-32768, 32768, (3, P, L)) | 0x4000).astype(np.int16)
    pcm[so[1]] = pcm[so[0]]                                                     # two identical loud rows
    gain[so[:3]] = 32767
    sel[so[:3], 0] = (1, 2, 255)
    if P > 1:
        sel[so[1], 1] = 0x80
    keep[so[5]] = 1
    bg = marks["big"]
    picks = rng.permutation(len(bg) - 1)[:min(len(bg) - 1, MAX_SELECTED)] + 1   # (member 0 is the kept row)
    sel[bg[picks], 0] = 1
    if P > 1:
        sel[bg[picks[:5]], 1] = 1
    if P > 2:
        sel[bg[picks[0]], 2:] = 1
    gain[bg[picks[:3]]] = (0, -5, 32767)
    keep[bg[0]] = 7
    keep[marks["kept"]] = 1 + np.arange(len(marks["kept"]))                     # (any non-zero value counts)
    sel[marks["steady"][1]] = 1
    sel[marks["loose"][:2]] = 1
    keep[marks["loose"][0]] = 1
    slots = np.cumsum(rng.integers(1, 4, n)).astype(np.int32) + 5
    return pcm, room, gain, n_rooms, sel, keep, slots, marks

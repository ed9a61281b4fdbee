"""Independent model of solo_mix_shared and solo_send_fanout (include/solo_mi355x.h), written from the rules of the interface, not from
solo_amd/csrc/solo_mix_shared.h / solo_fanout.h: numpy and plain Python loops.  The contributions, the energies and the selection order
come from the model of solo_mix (tests/mix_model.py); nothing here calls the library."""
import numpy as np

from mix_model import model_mix

INT32_MAX = 2 ** 31 - 1


def model_mix_shared(pcm, room, n_rooms, gain=None, max_speakers=3, keep=None, slots=None, fill=None):
    """pcm int16 [n, P, L], room int [n], gain int16 [n] / keep uint8 [n] / slots int [n] or None -> dict(pcm_spk [n,P,L], spk_list [n],
    spk_rows [n], pcm_room [n_rooms,P,L], room_list [n_rooms], source [n], energy [n,P], mixed [n,P], count).  fill: dict of arrays the
    outputs start from (copied), so what the call must not write keeps its fill.  A device refusal: count rows = -1, nothing else changes."""
    n, P, L = pcm.shape
    room = np.asarray(room).astype(np.int64)
    fill = fill or {}
    start = lambda k, shape, dt: np.zeros(shape, dt) if k not in fill else fill[k].copy()
    w = dict(pcm_spk=start("pcm_spk", (n, P, L), np.int16), spk_list=start("spk_list", (n,), np.int32), spk_rows=start("spk_rows", (n,), np.int32),
             pcm_room=start("pcm_room", (n_rooms, P, L), np.int16), room_list=start("room_list", (n_rooms,), np.int32),
             source=start("source", (n,), np.int32), energy=start("energy", (n, P), np.int64), mixed=start("mixed", (n, P), np.uint8))
    bad = bool(((room < -1) | (room >= n_rooms)).any())
    if slots is not None:
        s = np.asarray(slots).astype(np.int64)
        bad |= bool(s[0] < 0 or (np.diff(s) <= 0).any())
    if bad:
        w["count"] = dict(rows=-1, rooms=None, speakers=None, shared=None, clipped=None)
        return w
    assert 1 <= max_speakers <= 64
    base = model_mix(pcm[:n], room, n_rooms, gain, max_speakers, energy=w["energy"][:n], mixed=w["mixed"][:n])
    w["energy"][:n], w["mixed"][:n] = base["energy"], base["mixed"]
    flag = base["mixed"].astype(bool)
    member = room >= 0
    spk = member & (flag.any(axis=1) | (np.zeros(n, bool) if keep is None else np.asarray(keep) != 0))
    g = np.full(n, 4096, np.int64) if gain is None else np.maximum(np.asarray(gain).astype(np.int64), 0)
    c = (pcm.astype(np.int64) * g[:, None, None] + 2048) >> 12
    S = np.zeros((n_rooms, P, L), np.int64)
    for r in range(n_rooms):
        M = np.flatnonzero(room == r)
        for p in range(P):
            S[r, p] = c[M[flag[M, p]], p].sum(axis=0)
    clipped = 0
    rows = np.flatnonzero(spk)
    for k, i in enumerate(rows):
        o = S[room[i]] - np.where(flag[i][:, None], c[i], 0)
        clipped += int(((o > 32767) | (o < -32768)).sum())
        w["pcm_spk"][k] = np.clip(o, -32768, 32767)
        w["spk_rows"][k] = i
        w["spk_list"][k] = i if slots is None else slots[i]
        w["source"][i] = k
    shared = [r for r in range(n_rooms) if (member & ~spk & (room == r)).any()]
    for j, r in enumerate(shared):
        clipped += int(((S[r] > 32767) | (S[r] < -32768)).sum())
        w["pcm_room"][j] = np.clip(S[r], -32768, 32767)
        w["room_list"][j] = r
        w["source"][member & ~spk & (room == r)] = n + j
    w["source"][~member] = -1
    w["count"] = dict(rows=int(member.sum()), rooms=len(set(room[member].tolist())), speakers=len(rows), shared=len(shared), clipped=clipped)
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


def _datagrams(total, n1, slot, hbb, mask, seq):
    """the rules of solo_send_pack for one packet -> ("empty" | "refused" | "ok", len of MD1 or 0, len of MD2 || HB or 0)"""
    if total <= 0:
        return "empty", 0, 0
    if seq < 0 or seq > INT32_MAX or total > slot or n1 < 0 or n1 > total or 0 < n1 < hbb:
        return "refused", 0, 0
    return "ok", (total - n1 if mask & 1 and total - n1 > 0 else 0), (n1 if mask & 2 and n1 > hbb else 0)


def model_fanout(bits, nbytes, source, hbb, dst_stream=None, send=None, seq_base=None, first_seq=0, max_records=None, cap=None,
                 records=None, payload=None):
    """bits uint8 [n_src,P,slot], nbytes int16 [n_src,P,2], source int [n_dst] -> dict(records int32 [max,5], payload uint8 [cap], count,
    all_records: the uncapped list, pool: the uncapped pool).  records / payload: the arrays the outputs start from (copied; their sizes are
    the caps unless max_records / cap say otherwise).  A source outside [-1, n_src): count records = -1, nothing else changes."""
    n_src, P, slot = bits.shape
    source = np.asarray(source).astype(np.int64)
    n_dst = len(source)
    records = np.zeros((2 * n_dst * P, 5), np.int32) if records is None else records.copy()
    payload = np.zeros(n_src * P * slot, np.uint8) if payload is None else payload.copy()
    max_records = len(records) if max_records is None else max_records
    cap = min(len(payload) if cap is None else cap, INT32_MAX)
    if ((source < -1) | (source >= n_src)).any():
        return dict(records=records, payload=payload, count=dict(records=-1, records_needed=None, bytes=None, bytes_needed=None, empty=None, refused=None))
    named = set(int(s) for s in source if s >= 0)
    where, pool = {}, []                                         # (source row, packet, description) -> (offset, len)
    off = 0
    for p in range(P):
        for s in sorted(named):
            total, n1 = int(nbytes[s, p, 0]), int(nbytes[s, p, 1])
            what, l0, l1 = _datagrams(total, n1, slot, hbb, 3, 0)
            for d, (ln, at) in enumerate(((l0, 0), (l1, total - n1))):
                if ln:
                    where[s, p, d] = (off, ln)
                    pool.append(bits[s, p, at:at + ln])
                    off += ln
    pool = np.concatenate(pool) if pool else np.zeros(0, np.uint8)
    pool_written = 0
    for o, ln in where.values():
        if o + ln <= cap:
            pool_written = max(pool_written, o + ln)
    payload[:pool_written] = pool[:pool_written]
    allrec, empty, refused = [], 0, 0
    for p in range(P):
        for i in range(n_dst):
            s = int(source[i])
            if s < 0:
                continue
            seq = int(first_seq) + (0 if seq_base is None else int(seq_base[i])) + p
            what, l0, l1 = _datagrams(int(nbytes[s, p, 0]), int(nbytes[s, p, 1]), slot, hbb, 3 if send is None else int(send[i, p]) & 3, seq)
            empty += what == "empty"
            refused += what == "refused"
            for d, ln in enumerate((l0, l1)):
                if ln:
                    assert where[s, p, d][1] == ln
                    allrec.append((i if dst_stream is None else int(dst_stream[i]), seq, d, where[s, p, d][0], ln))
    written = 0
    for k, r in enumerate(allrec):
        if k < max_records and r[3] + r[4] <= cap:
            records[k] = r
            written += 1
    count = dict(records=written, records_needed=len(allrec), bytes=pool_written, bytes_needed=int(len(pool)), empty=int(empty), refused=int(refused))
    return dict(records=records, payload=payload, count=count, all_records=np.array(allrec, np.int64).reshape(-1, 5), pool=pool)


def shared_case(seed, P, L, max_speakers, big=70):
    """A floor with everything the interface of solo_mix_shared names, on top of mix_case (gains 0 / negative / 32767, full-scale rows that
    saturate, identical loud rows whose tie the row index decides, rows in no room): rooms of 1, 2, max_speakers, max_speakers + 1 (twice:
    the second one is kept whole by d_keep, so it is not shared), 9 and `big` members; in the room of 9 a row that is loudest in packet 0
    and silent afterwards; in the big room a silent row that d_keep makes a speaker; a kept row in no room (ignored); slots with gaps.
    -> (pcm, room, gain, n_rooms, keep uint8 [n], slots int32 [n], marks: dict of the rows named above)"""
    from mix_model import mix_case
    K = max_speakers
    sizes = (1, 2, K, K + 1, 9, big, K + 1)
    pcm, room, gain, n_rooms = mix_case(seed, P, L, sizes=sizes, loose=6)
    rng = np.random.default_rng(seed + 1)
    n = len(room)
    keep = np.zeros(n, np.uint8)
    keep[np.flatnonzero(room == 2 * 6)] = 1 + np.arange(K + 1) % 250            # (any non-zero value counts)
    nine, bigroom = np.flatnonzero(room == 2 * 4), np.flatnonzero(room == 2 * 5)
    once = int(nine[2])                                                       # (not one of mix_case's full-scale or identical rows)
    pcm[once] = 0
    pcm[once, 0] = -32768
    gain[once] = 32767
    silent = int(bigroom[4])
    pcm[silent] = 0
    keep[silent] = 1
    loose = np.flatnonzero(room < 0)
    keep[loose[0]] = 1
    slots = np.cumsum(rng.integers(1, 4, n)).astype(np.int32) + 5
    return pcm, room, gain, n_rooms, keep, slots, dict(once=once, silent=silent, kept_room=2 * 6, loose_kept=int(loose[0]))


def fanout_case(seed, n_src, n_dst, P, slot, hbb):
    """A source table and destinations with everything the interface of solo_send_fanout names.  Source rows: 0 = nobody names it, its length
    records are 0xA5 bytes; 1 = nobody names it, its records look valid; 2 = named, with DTX packets (total 0 and negative); 3 = named, one
    invalid record of every kind; 4 = named by two destinations and more; the others valid, with n1 = 0 (no second description) and n1 = hbb
    (high band alone) among them; the last row has one destination, which sends MD1 only.  Destinations: masks 0 .. 3, some with source -1, stream numbers and sequence bases of their own.
    -> (bits, nbytes, source int32 [n_dst], dst_stream int32 [n_dst], send uint8 [n_dst, P], seq_base int32 [n_dst])"""
    assert n_src >= 8 and n_dst >= 12 and P >= 1 and slot >= 4 * hbb + 8
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 256, (n_src, P, slot)).astype(np.uint8)
    total = rng.integers(2 * hbb + 2, slot + 1, (n_src, P))
    n1 = (total * rng.integers(30, 60, (n_src, P))) // 100
    n1[n1 <= hbb] = hbb + 1
    n1[5] = 0
    n1[6, 0::2] = hbb
    total[n_src - 1, 0] = slot                                                 # (a packet that fills its slot)
    nbytes = np.stack([total, n1], axis=-1).astype(np.int16)
    nbytes[0].view(np.uint8)[...] = 0xA5
    nbytes[2, 0::2] = (0, 9)
    nbytes[2, 1::2] = (-3, -3)
    for p, rec in enumerate([(slot + 1, hbb + 1), (40, -1), (40, 41), (40, hbb - 1), (-32768, 77)][:P]):
        nbytes[3, p] = rec
    source = rng.integers(2, n_src - 1, n_dst).astype(np.int32)
    source[:6] = (4, 3, 2, 4, -1, 4)
    source[-1] = -1
    source[-2] = n_src - 1                                                     # (its only destination, which sends MD1 alone)
    source[-3] = 5
    source[-4] = 6
    assert not ({0, 1} & set(source.tolist()))
    dst_stream = (np.cumsum(rng.integers(1, 3, n_dst)) + 3).astype(np.int32)
    send = rng.integers(0, 4, (n_dst, P)).astype(np.uint8)
    send[0], send[3], send[5] = 3, 1, 2
    send[6 % n_dst, 0] = 0
    send[-2] = 1
    send[rng.random((n_dst, P)) < 0.3] |= 0xF0                                    # (the upper bits do not count)
    seq_base = rng.integers(0, 1000, n_dst).astype(np.int32)
    return bits, nbytes, source, dst_stream, send, seq_base

"""Independent numpy model of solo_send_pack (include/solo_mi355x.h): what the CPU test compares the host build of solo_send.h with and
what the GPU tests compare the kernels with.  Written from the interface text, array-wise; it shares no code with the library."""
import numpy as np

REASONS = ("seq", "too_large", "n1_negative", "n1_over", "n1_short")
INT32_MAX = 2 ** 31 - 1


def model_pack(bits, nbytes, send, seq_base, first_seq, hbb, streams=None, max_records=None, cap=None):
    """bits uint8 [n,P,slot], nbytes int16 [n,P,2], send uint8 [n,P] or None, seq_base int [n] or None ->
    dict(records int32 [k,5], payload uint8 [bytes], count dict, reasons {name: packets}, all_records: the uncapped record list)"""
    n, P, slot = bits.shape
    total = nbytes[:, :, 0].astype(np.int64).T                  # [P][n]: the output order is packet-major
    n1 = nbytes[:, :, 1].astype(np.int64).T
    mask = np.full((P, n), 3, np.int64) if send is None else send.astype(np.int64).T & 3
    base = np.zeros(n, np.int64) if seq_base is None else np.asarray(seq_base).astype(np.int64)
    seq = int(first_seq) + base[None, :] + np.arange(P, dtype=np.int64)[:, None]
    empty = total <= 0
    why = {"seq": (seq < 0) | (seq > INT32_MAX), "too_large": total > slot, "n1_negative": n1 < 0, "n1_over": n1 > total,
           "n1_short": (n1 > 0) & (n1 < hbb)}
    refused = np.zeros_like(empty)
    for v in why.values():
        refused |= v & ~empty
    ok = ~empty & ~refused
    l0 = np.where(ok & ((mask & 1) != 0) & (total - n1 > 0), total - n1, 0)
    l1 = np.where(ok & ((mask & 2) != 0) & (n1 > hbb), n1, 0)
    lens = np.stack([l0, l1], axis=-1).reshape(-1)               # p, i, description
    offs = np.cumsum(lens) - lens
    rows = np.broadcast_to(np.arange(n, dtype=np.int64)[None, :, None], (P, n, 2)).reshape(-1)
    pkts = np.broadcast_to(np.arange(P, dtype=np.int64)[:, None, None], (P, n, 2)).reshape(-1)
    desc = np.broadcast_to(np.arange(2, dtype=np.int64)[None, None, :], (P, n, 2)).reshape(-1)
    src = (rows * P + pkts) * slot + np.where(desc == 1, (total - n1)[:, :, None].repeat(2, axis=2).reshape(-1), 0)
    sid = rows if streams is None else np.asarray(streams, np.int64)[rows]
    sel = lens > 0
    rec = np.stack([sid, np.broadcast_to(seq[:, :, None], (P, n, 2)).reshape(-1), desc, offs, lens], axis=1)[sel]
    src = src[sel]
    k = np.arange(rec.shape[0])
    lim = INT32_MAX if cap is None else min(int(cap), INT32_MAX)
    written = (rec[:, 3] + rec[:, 4] <= lim) & (k < (rec.shape[0] if max_records is None else max_records))
    nw = int(written.sum())
    assert written[:nw].all()                                   # a prefix
    wl = rec[:nw, 4]
    nbytes_w = int(wl.sum())
    idx = np.repeat(src[:nw] - rec[:nw, 3], wl) + np.arange(nbytes_w, dtype=np.int64)
    payload = bits.reshape(-1)[idx] if nbytes_w else np.zeros(0, np.uint8)
    count = dict(records=nw, records_needed=int(rec.shape[0]), bytes=nbytes_w, bytes_needed=int(lens.sum()), empty=int(empty.sum()),
                 refused=int(refused.sum()))
    return dict(records=rec[:nw].astype(np.int32), payload=payload, count=count, reasons={r: int((why[r] & ~empty).sum()) for r in REASONS},
                all_records=rec)

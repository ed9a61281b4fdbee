"""Independent numpy model of the stream-migration blob (include/solo_mi355x.h, solo_amd/csrc/solo_migrate.h): what an export must
write, what an import must accept and what it must leave behind.  Written from the format's description, not from the kernels."""
import numpy as np

MAGIC, VERSION, HDR = 0x4D474953, 1, 64
ENC, DEC, RECV = 1, 2, 4
TRK_WORDS, TRK_MARGIN = 10, 9
REASONS = dict(ok=0, list=1, magic=2, version=3, which=4, geometry=5, length=6, checksum=7, queue=8)
GEOM = ("enc_rate", "enc_mode", "enc_bytes", "dec_rate", "dec_mode", "dec_bytes", "depth", "slot")


def pad16(x):
    return (x + 15) // 16 * 16


def geom_words(g, which):
    """the eight geometry words of a blob with the sections `which`: zero for the sections it lacks"""
    w = [g[k] for k in GEOM]
    if not which & ENC:
        w[0:3] = [0, 0, 0]
    if not which & DEC:
        w[3:6] = [0, 0, 0]
    if not which & RECV:
        w[6:8] = [0, 0]
    return w


def section_bytes(gw, sec):
    if sec == ENC:
        return pad16(gw[2])
    if sec == DEC:
        return pad16(gw[5])
    D, slot = gw[6], gw[7]
    return 16 + pad16(4 * D) + pad16(2 * D * slot) + 48


def body_bytes(gw, which):
    return sum(section_bytes(gw, s) for s in (ENC, DEC, RECV) if which & s)


def section_offset(gw, which, sec):
    return sum(section_bytes(gw, s) for s in (ENC, DEC, RECV) if which & s and s < sec)


def state_bytes(g, which):
    return HDR + body_bytes(geom_words(g, which), which)


def checksums(body):
    """s1 = sum w_i, s2 = sum (i + 1) w_i, both mod 2^32, over the body's little-endian 32-bit words (exact integers)"""
    w = [int(x) for x in np.frombuffer(bytes(body), "<u4")]
    return sum(w) % 2 ** 32, sum((i + 1) * x for i, x in enumerate(w)) % 2 ** 32


def queue_section(h, s):
    """section 4 of stream s: play, length words and payload in play-relative order, bytes beyond `len` zero, the counters"""
    D, slot = h["g"]["depth"], h["g"]["slot"]
    p = int(h["play"][s])
    lens = np.array([h["lens"][s, (p + k) % D] for k in range(D)], np.uint32)
    pay = np.zeros((D, 2, slot), np.uint8)
    for k in range(D):
        e = (p + k) % D
        for d in range(2):
            n = (int(lens[k]) >> (16 * d)) & 0xFFFF
            pay[k, d, :n] = h["ring"][s, e, d, :n]
    trk = np.zeros(12, np.uint32)
    if h.get("trk") is not None:
        trk[:TRK_WORDS] = h["trk"][s]
    else:
        trk[TRK_MARGIN] = D
    out = np.zeros(section_bytes(geom_words(h["g"], RECV), RECV), np.uint8)
    out[0:4] = np.frombuffer(np.int32(p).tobytes(), np.uint8)
    out[16:16 + 4 * D] = lens.view(np.uint8)
    o = 16 + pad16(4 * D)
    out[o:o + 2 * D * slot] = pay.reshape(-1)
    o += pad16(2 * D * slot)
    out[o:o + 48] = trk.view(np.uint8)
    return out


def export_record(h, s, which):
    """one record: header + body, exactly state_bytes(g, which) bytes"""
    gw = geom_words(h["g"], which)
    parts = []
    if which & ENC:
        parts.append(np.pad(h["enc"][s], (0, pad16(gw[2]) - gw[2])))
    if which & DEC:
        parts.append(np.pad(h["dec"][s], (0, pad16(gw[5]) - gw[5])))
    if which & RECV:
        parts.append(queue_section(h, s))
    body = np.concatenate(parts).astype(np.uint8)
    s1, s2 = checksums(body)
    hd = np.array([MAGIC, VERSION, which, s] + gw + [body.size, s1, s2, 0], np.uint32)
    return np.concatenate([hd.view(np.uint8), body])


def check_record(row, g, which, stride):
    """the refusal rules, in the order the library documents them; returns a REASONS value"""
    hd = np.frombuffer(bytes(row[:HDR]), "<u4").astype(np.int64)
    if hd[0] != MAGIC:
        return REASONS["magic"]
    if hd[1] != VERSION:
        return REASONS["version"]
    bw = int(hd[2])
    if bw == 0 or bw > 7 or which & ~bw:
        return REASONS["which"]
    gw = [int(np.int32(np.uint32(x))) for x in hd[4:12]]
    hg = [g[k] for k in GEOM]
    if (which & ENC and gw[0:3] != hg[0:3]) or (which & DEC and gw[3:6] != hg[3:6]) or (which & RECV and gw[6:8] != hg[6:8]):
        return REASONS["geometry"]
    if gw[2] % 4 or gw[5] % 4 or not 0 <= gw[6] <= 4096 or not 0 <= gw[7] <= 0x7FFF:
        return REASONS["length"]
    mask = [gw[i] if bw & (ENC if i < 3 else DEC if i < 6 else RECV) else 0 for i in range(8)]
    mask[2], mask[5] = mask[2] & 0xFFFFFFFF, mask[5] & 0xFFFFFFFF
    body = body_bytes(mask, bw)
    if hd[12] != body or HDR + body > stride or hd[15] != 0:
        return REASONS["length"]
    if checksums(row[HDR:HDR + body]) != (int(hd[13]), int(hd[14])):
        return REASONS["checksum"]
    if which & RECV:
        o = HDR + section_offset(mask, bw, RECV)
        if int(np.frombuffer(bytes(row[o:o + 4]), "<i4")[0]) < 0:
            return REASONS["queue"]
        lens = np.frombuffer(bytes(row[o + 16:o + 16 + 4 * gw[6]]), "<u4")
        if ((lens & 0xFFFF) > gw[7]).any() or ((lens >> 16) > gw[7]).any():
            return REASONS["queue"]
    return REASONS["ok"]


def import_record(h, s, row, which):
    """the arrays of handle h after record `row` (already accepted) became stream s"""
    hd = np.frombuffer(bytes(row[:HDR]), "<u4")
    bw = int(hd[2])
    gw = [int(x) for x in hd[4:12]]
    if which & ENC:
        o = HDR + section_offset(gw, bw, ENC)
        h["enc"][s] = row[o:o + gw[2]]
    if which & DEC:
        o = HDR + section_offset(gw, bw, DEC)
        h["dec"][s] = row[o:o + gw[5]]
    if which & RECV:
        D, slot = gw[6], gw[7]
        o = HDR + section_offset(gw, bw, RECV)
        p = int(np.frombuffer(bytes(row[o:o + 4]), "<i4")[0])
        lens = np.frombuffer(bytes(row[o + 16:o + 16 + 4 * D]), "<u4")
        op = o + 16 + pad16(4 * D)
        pay = row[op:op + 2 * D * slot].reshape(D, 2, slot)
        h["play"][s] = p
        for k in range(D):
            e = (p + k) % D
            h["lens"][s, e] = lens[k]
            for d in range(2):
                n = (int(lens[k]) >> (16 * d)) & 0xFFFF
                h["ring"][s, e, d, :n] = pay[k, d, :n]
        if h.get("trk") is not None:
            ot = op + pad16(2 * D * slot)
            h["trk"][s] = np.frombuffer(bytes(row[ot:ot + 4 * TRK_WORDS]), "<u4")

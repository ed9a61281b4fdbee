// solo_migrate.h -- stream states leave a handle and enter another one: solo_batch_export_streams / solo_batch_import_streams
// (include/solo_mi355x.h).  A running call -- its encoder state, its decoder state, its receive queue -- is written into a versioned,
// checksummed DEVICE blob, one record per stream, and read back into any slot of any handle of the same geometry: on the same GPU,
// or, after the caller has sent the bytes, on another one.  The call goes on exactly where it stood: nothing is re-initialised.
//
// A BLOB IS VALID ONLY FOR THE LIBRARY BUILD THAT WROTE IT.  Sections 1 and 2 are the build's SxEncStream / SxDecStream records byte for
// byte; the header carries their sizes and an import refuses a record whose sizes differ.  It is a migration and standby format, not
// an archive format.
//
// Record (`blob_stride` bytes apart, a multiple of 16; base 16-byte aligned):
//
//     header, 16 words (64 bytes)
//        0 magic "SIGM"   1 version         2 which (1 encoder | 2 decoder | 4 receive queue)   3 origin stream index
//        4 enc samplerate 5 enc frames per packet | joint mode << 16    6 sizeof(SxEncStream)   7 dec samplerate
//        8 dec frames per packet | joint mode << 16    9 sizeof(SxDecStream)   10 ring depth    11 ring slot_bytes
//       12 body bytes    13 s1 = sum w_i           14 s2 = sum (i + 1) w_i     15 0
//       (words 4-6 / 7-9 / 10-11 are 0 without section 1 / 2 / 4; w_i: the body's 32-bit words, sums mod 2^32 -- both are
//        order-independent, so lanes keep partial sums with their own word indices and a wave reduction finishes them)
//     body: the sections in bit order, each padded with zeros to 16 bytes
//        1  the stream's SxEncStream        2  the stream's SxDecStream (SxDecState, the shadow, useMDIndex)
//        4  {play, 0, 0, 0} | D length words | D x 2 x slot payload bytes | 10 tracking counters, 0, 0
//           Length words and payload entries stand in PLAY-RELATIVE order: entry k belongs to sequence number play + k, so a blob does
//           not depend on where the ring's storage wraps.  Only the `len` bytes an entry's length word declares are copied; the rest of
//           a payload slot is written as zero, so equal queues give equal blobs.  The counters are those of solo_recv_track when the
//           handle ever allocated them, else zeros with margin_min = D; an import writes them only into a handle that has them.
//
// Kernels.  Export: a short kernel zeroes the three last header words of every record, then ONE WORKGROUP PER (record, section)
// copies its section with 16-byte loads and stores along the record, sums the words it stores, adds its two partial sums to the
// header and counts itself in; the workgroup that arrives last writes the rest of the header.  Import: ONE WAVEFRONT PER RECORD checks
// the header against the handle, recomputes both sums over the body and checks the queue's length words; any bad record sets the
// call's single verdict word (it keeps the FIRST bad record), and the copy kernel -- one workgroup per (record, section) again --
// leaves before it touches anything when that word or the list's is set: after a refused import every state of the handle is bit
// for bit what it was.  The stream records are only 4-byte aligned in general (sizeof(SxDecStream) is no multiple of 16), so their
// side of a copy is a 16-byte access at dword alignment; the blob's side and, with slot_bytes a multiple of 16, the ring's are
// 16-byte aligned.
//
// Everything outside the kernels compiles for the host as well (tests/test_migrate_model.py builds sx_mig_export_host /
// sx_mig_import_host, which walk records, sections and quads through the very functions of the kernels, and compares them with an
// independent numpy model).
#pragma once
#include "solo_recv.h"
#include "solo_wave.h"          // wg_sum
#include "solo_stream_ctl.h"

#define SX_MIG_MAGIC 0x4D474953u
#define SX_MIG_VERSION 1
#define SX_MIG_ENC 1
#define SX_MIG_DEC 2
#define SX_MIG_RECV 4
#define SX_MIG_ALL 7
#define SX_MIG_HDR_BYTES 64
// header words
#define SX_MIG_H_MAGIC 0
#define SX_MIG_H_VERSION 1
#define SX_MIG_H_WHICH 2
#define SX_MIG_H_ORIGIN 3
#define SX_MIG_H_GEOM 4         // eight words: SxMigGeom
#define SX_MIG_H_BODY 12
#define SX_MIG_H_S1 13
#define SX_MIG_H_S2 14
#define SX_MIG_H_ARRIVED 15     // sections written so far while an export runs; 0 in a finished blob
// why a record is refused
#define SX_MIG_OK 0
#define SX_MIG_BAD_LIST 1
#define SX_MIG_BAD_MAGIC 2
#define SX_MIG_BAD_VERSION 3
#define SX_MIG_BAD_WHICH 4      // the call asks for a section the blob does not hold
#define SX_MIG_BAD_GEOMETRY 5
#define SX_MIG_BAD_LENGTH 6
#define SX_MIG_BAD_SUM 7
#define SX_MIG_BAD_QUEUE 8      // a play-out position below 0 or a length above slot_bytes (a ring must never hold one)

typedef solo_migrate_count_t SxMigCount;
static_assert(sizeof(SxMigCount) == 16, "solo_migrate_count_t layout");

struct SxMigGeom {              // header words 4 .. 11: what a section's bytes mean; of a handle, or of a blob
    i32 enc_rate, enc_mode, enc_bytes, dec_rate, dec_mode, dec_bytes, depth, slot;
};
struct SxMigHandle {            // where a handle keeps what travels (a pointer is NULL without the direction / ring / counters)
    u8* enc; u8* dec; u8* ring; u32* lens; i32* play; u32* trk;
    SxMigGeom g;
    int n_streams;
};
struct alignas(16) SxMigQ { u32 x, y, z, w; };      // 16 bytes of a blob
struct SxMigQ4 { u32 x, y, z, w; };                 // 16 bytes of a stream record: dword aligned
struct SxMigSum { u32 s1, s2; };

SX_HD i64 sx_mig_pad16(i64 x) { return (x + 15) & ~(i64)15; }
SX_HD i32 sx_mig_mode(int frames_per_packet, int joint) { return frames_per_packet | (joint << 16); }
// the geometry words a blob with the sections `which` carries: those of the sections it lacks are 0
SX_HD SxMigGeom sx_mig_geom_of(const SxMigGeom& g, int which) {
    SxMigGeom r = g;
    if (!(which & SX_MIG_ENC)) { r.enc_rate = 0; r.enc_mode = 0; r.enc_bytes = 0; }
    if (!(which & SX_MIG_DEC)) { r.dec_rate = 0; r.dec_mode = 0; r.dec_bytes = 0; }
    if (!(which & SX_MIG_RECV)) { r.depth = 0; r.slot = 0; }
    return r;
}
// section 4: quads of its four parts
SX_HD i64 sx_mig_lens_quads(const SxMigGeom& g) { return sx_mig_pad16(4 * (i64)g.depth) >> 4; }
SX_HD i64 sx_mig_payload_quads(const SxMigGeom& g) { return sx_mig_pad16(2 * (i64)g.depth * (i64)g.slot) >> 4; }
#define SX_MIG_TRK_QUADS 3
// bytes of one section in the body (padded), of the body, and where a section starts in it
SX_HD i64 sx_mig_sec_bytes(const SxMigGeom& g, int sec) {
    if (sec == SX_MIG_ENC) return sx_mig_pad16((i64)(u32)g.enc_bytes);
    if (sec == SX_MIG_DEC) return sx_mig_pad16((i64)(u32)g.dec_bytes);
    return 16 * (1 + sx_mig_lens_quads(g) + sx_mig_payload_quads(g) + SX_MIG_TRK_QUADS);
}
SX_HD i64 sx_mig_sec_off(const SxMigGeom& g, int which, int sec) {
    i64 off = 0;
    for (int s = 1; s < sec; s <<= 1)
        if (which & s) off += sx_mig_sec_bytes(g, s);
    return off;
}
SX_HD i64 sx_mig_body_bytes(const SxMigGeom& g, int which) { return sx_mig_sec_off(g, which, 8); }
SX_HD int sx_mig_n_sections(int which) { return (which & 1) + ((which >> 1) & 1) + ((which >> 2) & 1); }
// the k-th section (k = 0 ..) of `which`
SX_HD int sx_mig_section(int which, int k) {
    for (int s = 1; s < 8; s <<= 1)
        if (which & s) { if (k == 0) return s; k--; }
    return 0;
}

// the body's words i0 .. i0 + 3
SX_HD void sx_mig_acc(SxMigSum* a, u32 i0, const SxMigQ& v) {
    a->s1 += v.x + v.y + v.z + v.w;
    a->s2 += (i0 + 1u) * v.x + (i0 + 2u) * v.y + (i0 + 3u) * v.z + (i0 + 4u) * v.w;
}

// ---- sections 1 and 2: quad q of a stream record of `bytes` bytes (a multiple of 4); behind the record: zeros / nothing written
SX_HD SxMigQ sx_mig_state_get(const u8* rec, u32 bytes, i64 q) {
    const i64 nw = bytes >> 2, w0 = 4 * q;
    const u32* w = (const u32*)rec + w0;
    SxMigQ v;
    if (w0 + 4 <= nw) {
        const SxMigQ4 t = *(const SxMigQ4*)w;
        v.x = t.x; v.y = t.y; v.z = t.z; v.w = t.w;
    } else {
        v.x = w0 < nw ? w[0] : 0u; v.y = w0 + 1 < nw ? w[1] : 0u; v.z = w0 + 2 < nw ? w[2] : 0u; v.w = 0u;
    }
    return v;
}
SX_HD void sx_mig_state_put(u8* rec, u32 bytes, i64 q, const SxMigQ& v) {
    const i64 nw = bytes >> 2, w0 = 4 * q;
    u32* w = (u32*)rec + w0;
    if (w0 + 4 <= nw) {
        SxMigQ4 t;
        t.x = v.x; t.y = v.y; t.z = v.z; t.w = v.w;
        *(SxMigQ4*)w = t;
    } else {
        if (w0 < nw) w[0] = v.x;
        if (w0 + 1 < nw) w[1] = v.y;
        if (w0 + 2 < nw) w[2] = v.z;
    }
}

// ---- section 4 -------------------------------------------------------------------------------------------------------------------
// the bytes at offset o .. o + 15 of the play-relative payload [D][2][slot] of stream s; lw(k): the length word of entry play + k
SX_HD u32 sx_mig_len_of(u32 lw, int desc) { return (lw >> (16 * desc)) & 0xFFFFu; }
SX_HD u32 sx_mig_keep_bytes(u32 w, i32 n) { return n >= 4 ? w : (n <= 0 ? 0u : (w & ((1u << (8 * n)) - 1u))); }
SX_HD SxMigQ sx_mig_payload_get(const SxMigHandle& h, int s, i32 play, i64 o) {
    const i64 D = h.g.depth, slot = h.g.slot, total = 2 * D * slot;
    SxMigQ v;
    v.x = v.y = v.z = v.w = 0u;
    if ((slot & 15) == 0 && ((uintptr_t)h.ring & 15) == 0) {           // the 16 bytes lie in one slot, aligned
        const i64 k = o / (2 * slot), rem = o - k * 2 * slot;
        const int desc = rem >= slot;
        const i32 j = (i32)(rem - desc * slot);
        const size_t e = sx_recv_entry(s, (i32)((u32)play + (u32)k), (int)D);
        const i32 valid = (i32)sx_mig_len_of(h.lens[e], desc) - j;
        if (valid > 0) {
            const SxMigQ t = *(const SxMigQ*)(h.ring + (e * 2 + (size_t)desc) * (size_t)slot + (size_t)j);
            v.x = sx_mig_keep_bytes(t.x, valid); v.y = sx_mig_keep_bytes(t.y, valid - 4);
            v.z = sx_mig_keep_bytes(t.z, valid - 8); v.w = sx_mig_keep_bytes(t.w, valid - 12);
        }
        return v;
    }
    u32 w[4] = {0u, 0u, 0u, 0u};
    for (int b = 0; b < 16 && o + b < total; b++) {
        const i64 k = (o + b) / (2 * slot), rem = (o + b) - k * 2 * slot;
        const int desc = rem >= slot;
        const i32 j = (i32)(rem - desc * slot);
        const size_t e = sx_recv_entry(s, (i32)((u32)play + (u32)k), (int)D);
        if (j < (i32)sx_mig_len_of(h.lens[e], desc)) w[b >> 2] |= (u32)h.ring[(e * 2 + (size_t)desc) * (size_t)slot + (size_t)j] << (8 * (b & 3));
    }
    v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
    return v;
}
// the same 16 bytes into the ring of stream s; blens: the blob's D length words (play-relative)
SX_HD void sx_mig_payload_put(const SxMigHandle& h, int s, i32 play, const u32* blens, i64 o, const SxMigQ& v) {
    const i64 D = h.g.depth, slot = h.g.slot, total = 2 * D * slot;
    if ((slot & 15) == 0 && ((uintptr_t)h.ring & 15) == 0) {
        const i64 k = o / (2 * slot), rem = o - k * 2 * slot;
        const int desc = rem >= slot;
        const i32 j = (i32)(rem - desc * slot);
        // (a whole quad inside the slot: the bytes behind `len` are not defined in a ring, the blob's zeros do no harm there)
        if (j < (i32)sx_mig_len_of(blens[k], desc))
            *(SxMigQ*)(h.ring + (sx_recv_entry(s, (i32)((u32)play + (u32)k), (int)D) * 2 + (size_t)desc) * (size_t)slot + (size_t)j) = v;
        return;
    }
    const u32 w[4] = {v.x, v.y, v.z, v.w};
    for (int b = 0; b < 16 && o + b < total; b++) {
        const i64 k = (o + b) / (2 * slot), rem = (o + b) - k * 2 * slot;
        const int desc = rem >= slot;
        const i32 j = (i32)(rem - desc * slot);
        if (j < (i32)sx_mig_len_of(blens[k], desc))
            h.ring[(sx_recv_entry(s, (i32)((u32)play + (u32)k), (int)D) * 2 + (size_t)desc) * (size_t)slot + (size_t)j] = (u8)(w[b >> 2] >> (8 * (b & 3)));
    }
}
// quad q of section 4 of stream s
SX_HD SxMigQ sx_mig_ring_get(const SxMigHandle& h, int s, i64 q) {
    const i64 L = sx_mig_lens_quads(h.g), P = sx_mig_payload_quads(h.g);
    const i32 play = h.play[s];
    SxMigQ v;
    v.x = v.y = v.z = v.w = 0u;
    if (q == 0) {
        v.x = (u32)play;
    } else if (q < 1 + L) {
        const i64 k = 4 * (q - 1);
        const u32* l = h.lens;
        const int D = h.g.depth;
        v.x = k < D ? l[sx_recv_entry(s, (i32)((u32)play + (u32)k), D)] : 0u;
        v.y = k + 1 < D ? l[sx_recv_entry(s, (i32)((u32)play + (u32)k + 1u), D)] : 0u;
        v.z = k + 2 < D ? l[sx_recv_entry(s, (i32)((u32)play + (u32)k + 2u), D)] : 0u;
        v.w = k + 3 < D ? l[sx_recv_entry(s, (i32)((u32)play + (u32)k + 3u), D)] : 0u;
    } else if (q < 1 + L + P) {
        v = sx_mig_payload_get(h, s, play, 16 * (q - 1 - L));
    } else {
        const int t = (int)(q - 1 - L - P) * 4;
        u32 w[4];
        for (int c = 0; c < 4; c++) {
            const int i = t + c;
            w[c] = i >= SX_RECV_TRK_WORDS ? 0u : (h.trk ? h.trk[(size_t)s * SX_RECV_TRK_WORDS + i] : (i == SX_RECV_TRK_MARGIN ? (u32)h.g.depth : 0u));
        }
        v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
    }
    return v;
}
// sec4: the blob's section 4 (its head and length words are read from there; the geometry is the handle's: checked before)
SX_HD void sx_mig_ring_put(const SxMigHandle& h, int s, const u8* sec4, i64 q, const SxMigQ& v) {
    const i64 L = sx_mig_lens_quads(h.g), P = sx_mig_payload_quads(h.g);
    const i32 play = *(const i32*)sec4;
    const u32* blens = (const u32*)(sec4 + 16);
    const int D = h.g.depth;
    if (q == 0) {
        h.play[s] = play;
    } else if (q < 1 + L) {
        const i64 k = 4 * (q - 1);
        if (k < D) h.lens[sx_recv_entry(s, (i32)((u32)play + (u32)k), D)] = v.x;
        if (k + 1 < D) h.lens[sx_recv_entry(s, (i32)((u32)play + (u32)k + 1u), D)] = v.y;
        if (k + 2 < D) h.lens[sx_recv_entry(s, (i32)((u32)play + (u32)k + 2u), D)] = v.z;
        if (k + 3 < D) h.lens[sx_recv_entry(s, (i32)((u32)play + (u32)k + 3u), D)] = v.w;
    } else if (q < 1 + L + P) {
        sx_mig_payload_put(h, s, play, blens, 16 * (q - 1 - L), v);
    } else if (h.trk) {
        const int t = (int)(q - 1 - L - P) * 4;
        const u32 w[4] = {v.x, v.y, v.z, v.w};
        for (int c = 0; c < 4; c++)
            if (t + c < SX_RECV_TRK_WORDS) h.trk[(size_t)s * SX_RECV_TRK_WORDS + t + c] = w[c];
    }
}

// quad q of section `sec` of stream s, out of the handle / into it
SX_HD SxMigQ sx_mig_get(const SxMigHandle& h, int sec, int s, i64 q) {
    if (sec == SX_MIG_ENC) return sx_mig_state_get(h.enc + (size_t)s * (size_t)(u32)h.g.enc_bytes, (u32)h.g.enc_bytes, q);
    if (sec == SX_MIG_DEC) return sx_mig_state_get(h.dec + (size_t)s * (size_t)(u32)h.g.dec_bytes, (u32)h.g.dec_bytes, q);
    return sx_mig_ring_get(h, s, q);
}
SX_HD void sx_mig_put(const SxMigHandle& h, int sec, int s, const u8* sec_base, i64 q, const SxMigQ& v) {
    if (sec == SX_MIG_ENC) sx_mig_state_put(h.enc + (size_t)s * (size_t)(u32)h.g.enc_bytes, (u32)h.g.enc_bytes, q, v);
    else if (sec == SX_MIG_DEC) sx_mig_state_put(h.dec + (size_t)s * (size_t)(u32)h.g.dec_bytes, (u32)h.g.dec_bytes, q, v);
    else sx_mig_ring_put(h, s, sec_base, q, v);
}

// the header of a record that holds the sections `which` of stream `origin` (the sums and word 15 are the copy kernel's)
SX_HD void sx_mig_header(u32* hd, const SxMigGeom& g, int which, int origin) {
    const SxMigGeom bg = sx_mig_geom_of(g, which);
    hd[SX_MIG_H_MAGIC] = SX_MIG_MAGIC; hd[SX_MIG_H_VERSION] = SX_MIG_VERSION; hd[SX_MIG_H_WHICH] = (u32)which; hd[SX_MIG_H_ORIGIN] = (u32)origin;
    hd[4] = (u32)bg.enc_rate; hd[5] = (u32)bg.enc_mode; hd[6] = (u32)bg.enc_bytes; hd[7] = (u32)bg.dec_rate;
    hd[8] = (u32)bg.dec_mode; hd[9] = (u32)bg.dec_bytes; hd[10] = (u32)bg.depth; hd[11] = (u32)bg.slot;
    hd[SX_MIG_H_BODY] = (u32)sx_mig_body_bytes(bg, which);
}
SX_HD SxMigGeom sx_mig_header_geom(const u32* hd) {
    SxMigGeom g;
    g.enc_rate = (i32)hd[4]; g.enc_mode = (i32)hd[5]; g.enc_bytes = (i32)hd[6]; g.dec_rate = (i32)hd[7];
    g.dec_mode = (i32)hd[8]; g.dec_bytes = (i32)hd[9]; g.depth = (i32)hd[10]; g.slot = (i32)hd[11];
    return g;
}
// Everything of a record that its header alone decides; g: the handle's geometry, which: what the call wants to import.  A record
// that passes can be walked: its body lies inside the stride and its section offsets follow from its own header.
SX_HD int sx_mig_check_header(const u32* hd, const SxMigGeom& g, int which, i64 stride) {
    if (hd[SX_MIG_H_MAGIC] != SX_MIG_MAGIC) return SX_MIG_BAD_MAGIC;
    if (hd[SX_MIG_H_VERSION] != SX_MIG_VERSION) return SX_MIG_BAD_VERSION;
    const u32 bw = hd[SX_MIG_H_WHICH];
    if (bw == 0 || bw > SX_MIG_ALL || ((u32)which & ~bw)) return SX_MIG_BAD_WHICH;
    const SxMigGeom bg = sx_mig_header_geom(hd);
    if ((which & SX_MIG_ENC) && (bg.enc_rate != g.enc_rate || bg.enc_mode != g.enc_mode || bg.enc_bytes != g.enc_bytes)) return SX_MIG_BAD_GEOMETRY;
    if ((which & SX_MIG_DEC) && (bg.dec_rate != g.dec_rate || bg.dec_mode != g.dec_mode || bg.dec_bytes != g.dec_bytes)) return SX_MIG_BAD_GEOMETRY;
    if ((which & SX_MIG_RECV) && (bg.depth != g.depth || bg.slot != g.slot)) return SX_MIG_BAD_GEOMETRY;
    // (sections the call does not take still decide where the others lie: their sizes must at least be sizes)
    if ((bg.enc_bytes & 3) || (bg.dec_bytes & 3) || bg.depth < 0 || bg.depth > 4096 || bg.slot < 0 || bg.slot > 0x7FFF) return SX_MIG_BAD_LENGTH;
    const i64 body = sx_mig_body_bytes(sx_mig_geom_of(bg, (int)bw), (int)bw);
    if ((i64)hd[SX_MIG_H_BODY] != body || SX_MIG_HDR_BYTES + body > stride || hd[SX_MIG_H_ARRIVED] != 0u) return SX_MIG_BAD_LENGTH;
    return SX_MIG_OK;
}
// position i of the stream list
SX_HD int sx_mig_list_bad(const i32* map, int i, int n_streams) { return map[i] < 0 || map[i] >= n_streams || (i > 0 && map[i - 1] >= map[i]); }

// One record of an import, by the lanes of ONE wavefront (the host form has one lane): the header, both sums over the body, and
// with section 4 the queue's own words.  Returns the reason in every lane.
SX_HD int sx_mig_check_record(const u8* row, const SxMigGeom& g, int which, i64 stride) {
    const u32* hd = (const u32*)row;
    const int why = sx_mig_check_header(hd, g, which, stride);
    if (why != SX_MIG_OK) return why;
    const i64 nq = (i64)hd[SX_MIG_H_BODY] >> 4;
    const SxMigQ* body = (const SxMigQ*)(row + SX_MIG_HDR_BYTES);
    SxMigSum a;
    a.s1 = 0u; a.s2 = 0u;
    for (i64 q = SX_LANE; q < nq; q += SX_NLANES) sx_mig_acc(&a, (u32)(4 * q), body[q]);
    const u32 s1 = (u32)wv_sum((i32)a.s1), s2 = (u32)wv_sum((i32)a.s2);
    if (s1 != hd[SX_MIG_H_S1] || s2 != hd[SX_MIG_H_S2]) return SX_MIG_BAD_SUM;
    i32 bad = 0;
    if (which & SX_MIG_RECV) {
        const u8* sec4 = row + SX_MIG_HDR_BYTES + sx_mig_sec_off(sx_mig_header_geom(hd), (int)hd[SX_MIG_H_WHICH], SX_MIG_RECV);
        if (*(const i32*)sec4 < 0) bad = 1;
        const u32* blens = (const u32*)(sec4 + 16);
        for (int k = SX_LANE; k < g.depth; k += SX_NLANES)
            if ((i32)sx_mig_len_of(blens[k], 0) > g.slot || (i32)sx_mig_len_of(blens[k], 1) > g.slot) bad = 1;
        bad = wv_max(bad);
    }
    return bad ? SX_MIG_BAD_QUEUE : SX_MIG_OK;
}

#if defined(__HIPCC__)
// export, ahead of the copy: the sums and the arrival count of every record start at 0
__global__ void __launch_bounds__(256) solo_migrate_prepare_kernel(u8* blob, long long stride, int n, const i32* map, const u32* verdict) {
    if (sx_map_refused(map, verdict)) return;
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= n) return;
    u32* hd = (u32*)(blob + (size_t)i * (size_t)stride);
    hd[SX_MIG_H_S1] = 0u; hd[SX_MIG_H_S2] = 0u; hd[SX_MIG_H_ARRIVED] = 0u;
}

// export: workgroup (record, k) copies the k-th section of `which` of stream map[record]
__global__ void __launch_bounds__(256) solo_migrate_export_kernel(const SxMigHandle h, const i32* __restrict__ map, int n, int which, u8* __restrict__ blob,
                                                                  long long stride, SxMigCount* count, const u32* verdict) {
    __shared__ i32 red[4];
    if (sx_map_refused(map, verdict)) {
        if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) count->streams = -1;
        return;
    }
    const int rec = (int)blockIdx.x, sec = sx_mig_section(which, (int)blockIdx.y), s = map[rec];
    const SxMigGeom bg = sx_mig_geom_of(h.g, which);
    const i64 off = sx_mig_sec_off(bg, which, sec), nq = sx_mig_sec_bytes(bg, sec) >> 4;
    u8* row = blob + (size_t)rec * (size_t)stride;
    SxMigQ* out = (SxMigQ*)(row + SX_MIG_HDR_BYTES + off);
    SxMigSum a;
    a.s1 = 0u; a.s2 = 0u;
    for (i64 q = threadIdx.x; q < nq; q += 256) {
        const SxMigQ v = sx_mig_get(h, sec, s, q);
        out[q] = v;
        sx_mig_acc(&a, (u32)((off >> 2) + 4 * q), v);
    }
    const u32 s1 = (u32)wg_sum((i32)a.s1, red), s2 = (u32)wg_sum((i32)a.s2, red);
    if (threadIdx.x == 0) {
        u32* hd = (u32*)row;
        atomicAdd(&hd[SX_MIG_H_S1], s1);
        atomicAdd(&hd[SX_MIG_H_S2], s2);
        __threadfence();
        // (wrapping adds in any order give the same sums; the section that counts itself in last finishes the header)
        if (atomicAdd(&hd[SX_MIG_H_ARRIVED], 1u) == (u32)sx_mig_n_sections(which) - 1u) {
            sx_mig_header(hd, h.g, which, s);
            hd[SX_MIG_H_ARRIVED] = 0u;
        }
        if (rec == 0 && blockIdx.y == 0) {
            SxMigCount c;
            c.streams = n; c.refused = 0; c.bytes = (i64)n * (SX_MIG_HDR_BYTES + sx_mig_body_bytes(bg, which));
            *count = c;
        }
    }
}

// import, first kernel: wavefront i checks record i and list position i; bad[0] (zeroed by the call) keeps n - (the first bad index)
__global__ void __launch_bounds__(64) solo_migrate_check_kernel(const SxMigGeom g, int n_streams, const i32* __restrict__ map, int n, int which,
                                                                const u8* __restrict__ blob, long long stride, u32* bad) {
    const int i = (int)blockIdx.x;
    int why = sx_mig_list_bad(map, i, n_streams) ? SX_MIG_BAD_LIST : SX_MIG_OK;
    if (why == SX_MIG_OK) why = sx_mig_check_record(blob + (size_t)i * (size_t)stride, g, which, stride);
    if (why != SX_MIG_OK && threadIdx.x == 0) atomicMax(bad, (u32)(n - i));
}

// import, second kernel: workgroup (record, k) copies the k-th section of `which` into stream map[record]; verdict[0]: the list's,
// verdict[1]: the records'
__global__ void __launch_bounds__(256) solo_migrate_import_kernel(const SxMigHandle h, const i32* __restrict__ map, int n, int which, const u8* __restrict__ blob,
                                                                  long long stride, SxMigCount* count, const u32* verdict) {
    const u32 bad = (u32)__builtin_amdgcn_readfirstlane((int)verdict[1]);
    if (bad != 0u || sx_map_refused(map, verdict)) {
        if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
            SxMigCount c;
            c.streams = -1; c.refused = bad ? n - (i32)bad + 1 : 0; c.bytes = 0;
            *count = c;
        }
        return;
    }
    const int rec = (int)blockIdx.x, sec = sx_mig_section(which, (int)blockIdx.y), s = map[rec];
    const u8* row = blob + (size_t)rec * (size_t)stride;
    const u32* hd = (const u32*)row;
    const SxMigGeom bg = sx_mig_header_geom(hd);             // (where the sections lie is the blob's business: it may hold more than the call takes)
    const u8* base = row + SX_MIG_HDR_BYTES + sx_mig_sec_off(bg, (int)hd[SX_MIG_H_WHICH], sec);
    const i64 nq = sx_mig_sec_bytes(bg, sec) >> 4;
    const SxMigQ* in = (const SxMigQ*)base;
    for (i64 q = threadIdx.x; q < nq; q += 256) sx_mig_put(h, sec, s, base, q, in[q]);
    if (rec == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        SxMigCount c;
        c.streams = n; c.refused = 0; c.bytes = (i64)n * (SX_MIG_HDR_BYTES + sx_mig_body_bytes(sx_mig_geom_of(h.g, which), which));     // (what was taken)
        *count = c;
    }
}

static inline hipError_t solo_migrate_export_launch(const SxMigHandle& h, const i32* map, int n, int which, u8* blob, long long stride, SxMigCount* count,
                                                    const u32* verdict, hipStream_t s) {
    hipLaunchKernelGGL(solo_migrate_prepare_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, blob, stride, n, map, verdict);
    hipLaunchKernelGGL(solo_migrate_export_kernel, dim3((unsigned)n, (unsigned)sx_mig_n_sections(which)), dim3(256), 0, s, h, map, n, which, blob, stride, count,
                       verdict);
    return hipGetLastError();
}
// verdict: two words, [0] written by the list check ahead of this, [1] zeroed here
static inline hipError_t solo_migrate_import_launch(const SxMigHandle& h, const i32* map, int n, int which, const u8* blob, long long stride, SxMigCount* count,
                                                    u32* verdict, hipStream_t s) {
    const hipError_t e = hipMemsetAsync(verdict + 1, 0, sizeof(u32), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(solo_migrate_check_kernel, dim3((unsigned)n), dim3(64), 0, s, h.g, h.n_streams, map, n, which, blob, stride, verdict + 1);
    hipLaunchKernelGGL(solo_migrate_import_kernel, dim3((unsigned)n, (unsigned)sx_mig_n_sections(which)), dim3(256), 0, s, h, map, n, which, blob, stride, count,
                       verdict);
    return hipGetLastError();
}
#else
// Host forms (tests): record by record, section by section, quad by quad through the functions above.
static inline int sx_mig_list_refused(const i32* map, int n, int n_streams) {
    for (int i = 0; i < n; i++)
        if (sx_mig_list_bad(map, i, n_streams)) return 1;
    return 0;
}
static inline void sx_mig_export_host(const SxMigHandle& h, const i32* map, int n, int which, u8* blob, long long stride, SxMigCount* count) {
    if (sx_mig_list_refused(map, n, h.n_streams)) { count->streams = -1; return; }
    const SxMigGeom bg = sx_mig_geom_of(h.g, which);
    for (int rec = 0; rec < n; rec++) {
        u8* row = blob + (size_t)rec * (size_t)stride;
        u32* hd = (u32*)row;
        SxMigSum a;
        a.s1 = 0u; a.s2 = 0u;
        for (int k = 0; k < sx_mig_n_sections(which); k++) {
            const int sec = sx_mig_section(which, k);
            const i64 off = sx_mig_sec_off(bg, which, sec), nq = sx_mig_sec_bytes(bg, sec) >> 4;
            SxMigQ* out = (SxMigQ*)(row + SX_MIG_HDR_BYTES + off);
            for (i64 q = 0; q < nq; q++) {
                const SxMigQ v = sx_mig_get(h, sec, map[rec], q);
                out[q] = v;
                sx_mig_acc(&a, (u32)((off >> 2) + 4 * q), v);
            }
        }
        sx_mig_header(hd, h.g, which, map[rec]);
        hd[SX_MIG_H_S1] = a.s1; hd[SX_MIG_H_S2] = a.s2; hd[SX_MIG_H_ARRIVED] = 0u;
    }
    count->streams = n; count->refused = 0; count->bytes = (i64)n * (SX_MIG_HDR_BYTES + sx_mig_body_bytes(bg, which));
}
// *why (may be NULL): the reason the first bad record was refused for
static inline void sx_mig_import_host(const SxMigHandle& h, const i32* map, int n, int which, const u8* blob, long long stride, SxMigCount* count, int* why_out) {
    for (int i = 0; i < n; i++) {
        int why = sx_mig_list_bad(map, i, h.n_streams) ? SX_MIG_BAD_LIST : SX_MIG_OK;
        if (why == SX_MIG_OK) why = sx_mig_check_record(blob + (size_t)i * (size_t)stride, h.g, which, stride);
        if (why != SX_MIG_OK) {
            count->streams = -1; count->refused = i + 1; count->bytes = 0;
            if (why_out) *why_out = why;
            return;
        }
    }
    if (why_out) *why_out = SX_MIG_OK;
    for (int rec = 0; rec < n; rec++) {
        const u8* row = blob + (size_t)rec * (size_t)stride;
        const u32* hd = (const u32*)row;
        const SxMigGeom bg = sx_mig_header_geom(hd);
        for (int k = 0; k < sx_mig_n_sections(which); k++) {
            const int sec = sx_mig_section(which, k);
            const u8* base = row + SX_MIG_HDR_BYTES + sx_mig_sec_off(bg, (int)hd[SX_MIG_H_WHICH], sec);
            const i64 nq = sx_mig_sec_bytes(bg, sec) >> 4;
            for (i64 q = 0; q < nq; q++) sx_mig_put(h, sec, map[rec], base, q, ((const SxMigQ*)base)[q]);
        }
    }
    count->streams = n; count->refused = 0; count->bytes = (i64)n * (SX_MIG_HDR_BYTES + sx_mig_body_bytes(sx_mig_geom_of(h.g, which), which));
}
#endif

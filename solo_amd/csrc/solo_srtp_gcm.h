// solo_srtp_gcm.h -- AEAD_AES_128_GCM (RFC 7714) for the SRTP and the SRTCP stage, beside the AES-CM / HMAC-SHA1 transforms of solo_srtp.h and
// solo_srtcp.h: the same four device calls, the same key records, one transform per stream and direction -- that of the key set last.
// A key record whose `transform` word is SX_SRTP_GCM holds the round keys, the 12 salt bytes in salt[0 .. 2], H = AES_k(0^128) in
// mid_i[0 .. 3] and tag = 16.  The kernels of the two older headers leave a datagram under such a key alone (SX_SRTP_ELSEWHERE); the
// kernels below run behind them, take exactly those datagrams and add to the same count, so every datagram is counted once.
//
//     SRTP    IV = (00 00 || SSRC || ROC || SEQ) ^ salt; AAD = the RTP header (what AES-CM leaves in the clear); wire: header, ciphertext, tag
//     SRTCP   IV = (00 00 || SSRC || 00 00 || index) ^ salt; E = 1: AAD = bytes [0, 8) || the E || index word, plaintext [8, len);
//             E = 0 (accepted, never written): AAD = the packet || the word, nothing encrypted; wire: packet, tag (16), THEN the word
//     GCM     J0 = IV || 00 00 00 01, keystream block j = AES_k(IV || be32(j + 2)), tag = AES_k(J0) ^ GHASH(H, AAD, ciphertext)
//
// GHASH.  gfx950 has no carry-less multiply, so Y = (Y ^ X) . H is the 4-bit table method (Shoup): the 16 multiples M[e] of H by the
// polynomials of degree < 4, and per block 32 steps  Z = (Z >> 4) ^ R[the four bits shifted out] ^ M[nibble], from the last nibble of the
// block to the first; R is the 16-entry reduction table (the right-shift form of SP 800-38D: R = 0xE1 || 0^120).  A step is four LDS
// words, a 128-bit shift and four XORs, about a quarter of the bit-serial count.  The table of a datagram's key is built by the datagram's
// lane into LDS ([entry][word][lane]: the lanes of a wave read 64 consecutive dwords, no bank conflict; 256 B a lane), which bounds the
// tile: 256 lanes x 256 B would be all of the 64 KB a workgroup may declare statically, so SX_GCM_TILE = 64 datagrams = 16 KB of tables;
// at 19 584 bytes a workgroup the 160 KB of a gfx950 CU's LDS hold eight of these one-wave workgroups, two a SIMD.  Building costs three
// doublings and eleven XORs of four words: nothing beside the 32 steps of even one block, so no per-key table is kept in memory.
// The accumulator and a table entry are four words at constant indices; nothing goes to scratch.
//
// The cut stays that of solo_srtp.h with the smaller tile:
//     protect    plan, table (a lane per datagram) | barrier | cipher (a 16-lane row per datagram) | barrier | GHASH over the ciphertext,
//                tag, d_dgrams (a lane per datagram)
//     unprotect  plan, table, GHASH, compare (a lane per datagram) | barrier | cipher for the accepted datagrams
// Everything below compiles for the host as well (tests/test_srtp_gcm_model.py).
#pragma once
#include "solo_srtcp.h"

#define SX_GCM_TAG SOLO_SRTP_GCM_TAG_BYTES
#define SX_SRTCP_GCM_TRAILER SOLO_SRTCP_GCM_TRAILER_BYTES
#define SX_GCM_MASTER SOLO_SRTP_GCM_MASTER_BYTES
#define SX_GCM_TILE 64          // datagrams per workgroup of the four kernels below
#define SX_GCM_TABLE_WORDS 64   // 16 entries of four words
static_assert(SX_GCM_TAG == 16 && SX_SRTCP_GCM_TRAILER == SX_GCM_TAG + 4 && SX_GCM_MASTER == 16 + 12, "tag, then the E || index word; key || salt");
static_assert(SX_GCM_TILE % SX_RTP_ROW == 0 && SX_GCM_TILE <= SX_RTP_TILE, "whole rows");

// R[r] << 16: what the four bits r shifted out of Z's low end fold back into its first word
#define SX_GCM_RED_LIST 0x00000000u, 0x1C200000u, 0x38400000u, 0x24600000u, 0x70800000u, 0x6CA00000u, 0x48C00000u, 0x54E00000u, \
                        0xE1000000u, 0xFD200000u, 0xD9400000u, 0xC5600000u, 0x91800000u, 0x8DA00000u, 0xA9C00000u, 0xB5E00000u
static const u32 SX_GCM_RED[16] = {SX_GCM_RED_LIST};
#if defined(__HIPCC__)
__device__ static const u32 SX_GCM_RED_DEV[16] = {SX_GCM_RED_LIST};
#endif

// ---- GF(2^128): a block is four big-endian words, the leftmost bit of word 0 the coefficient of x^0 -----------------------------------------
// tab[(4 e + w) * stride] = word w of H . (the polynomial whose coefficients of x^0 .. x^3 are bits 3 .. 0 of e)
SX_HD void sx_gcm_table(const u32* h, u32* tab, int stride) {
    u32 v0 = h[0], v1 = h[1], v2 = h[2], v3 = h[3];
#pragma unroll
    for (int w = 0; w < 4; w++) tab[w * stride] = 0;
#pragma unroll
    for (int e = 8; e > 0; e >>= 1) {                       // 8: H; 4: H x; 2: H x^2; 1: H x^3
        tab[(4 * e + 0) * stride] = v0; tab[(4 * e + 1) * stride] = v1; tab[(4 * e + 2) * stride] = v2; tab[(4 * e + 3) * stride] = v3;
        const u32 carry = v3 & 1u;
        v3 = (v3 >> 1) | (v2 << 31); v2 = (v2 >> 1) | (v1 << 31); v1 = (v1 >> 1) | (v0 << 31); v0 = (v0 >> 1) ^ (carry ? 0xE1000000u : 0u);
    }
#pragma unroll
    for (int e = 2; e <= 8; e *= 2)
#pragma unroll
        for (int j = 1; j < e; j++)
#pragma unroll
            for (int w = 0; w < 4; w++) tab[(4 * (e + j) + w) * stride] = tab[(4 * e + w) * stride] ^ tab[(4 * j + w) * stride];
}
// y = y . H
SX_HD void sx_gcm_mul(u32* y, const u32* tab, int stride, const u32* red) {
    const u32 x[4] = {y[0], y[1], y[2], y[3]};
    u32 z0 = 0, z1 = 0, z2 = 0, z3 = 0;
#pragma unroll
    for (int w = 3; w >= 0; w--) {
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const u32 e = (x[w] >> (4 * k)) & 15u, r = red[z3 & 15u];
            const u32* m = tab + 4 * e * stride;
            z3 = ((z3 >> 4) | (z2 << 28)) ^ m[3 * stride];
            z2 = ((z2 >> 4) | (z1 << 28)) ^ m[2 * stride];
            z1 = ((z1 >> 4) | (z0 << 28)) ^ m[1 * stride];
            z0 = (z0 >> 4) ^ r ^ m[0];
        }
    }
    y[0] = z0; y[1] = z1; y[2] = z2; y[3] = z3;
}
// the big-endian word at byte b of  p[0 .. n) || the first n_word bytes of `word` (big-endian) || zeros
SX_HD u32 sx_gcm_aad_word(const u8* p, i32 n, u32 word, i32 n_word, i32 b) {
    if (b + 4 <= n) return sx_rtp_be32(p + b, p, p + n);
    u32 v = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const i32 at = b + k;
        u32 x = 0;
        if (at < n) x = p[at];
        else if (at < n + n_word) x = (word >> (8 * (3 - (at - n)))) & 255u;
        v = (v << 8) | x;
    }
    return v;
}
// GHASH(H, A, C) by ONE lane: A = aad[0 .. n_aad) || the first n_word bytes of word, C = ct[0 .. n_ct); loads are clipped to the two ranges
SX_HD void sx_gcm_ghash(const u32* tab, int stride, const u32* red, const u8* aad, i32 n_aad, u32 word, i32 n_word, const u8* ct, i32 n_ct, u32* y) {
    y[0] = y[1] = y[2] = y[3] = 0;
    const i32 n_a = n_aad + n_word;
    for (i32 b = 0; b < n_a; b += 16) {
#pragma unroll
        for (int k = 0; k < 4; k++) y[k] ^= sx_gcm_aad_word(aad, n_aad, word, n_word, b + 4 * k);
        sx_gcm_mul(y, tab, stride, red);
    }
    for (i32 b = 0; b < n_ct; b += 16) {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (b + 4 * k < n_ct) y[k] ^= sx_rtp_be32(ct + b + 4 * k, ct, ct + n_ct);
        sx_gcm_mul(y, tab, stride, red);
    }
    y[1] ^= 8u * (u32)n_a; y[3] ^= 8u * (u32)n_ct;         // [8 len(A)]_64 || [8 len(C)]_64: both below 2^32
    sx_gcm_mul(y, tab, stride, red);
}
// the first three words of J0 and of every counter block; with (roc, seq) = (index >> 16, index & 0xFFFF) this is SRTCP's IV as well
SX_HD void sx_gcm_iv(const SxSrtpKey* key, u32 ssrc, u32 roc, u32 seq, u32* iv) {
    iv[0] = key->salt[0] ^ (ssrc >> 16); iv[1] = key->salt[1] ^ (ssrc << 16) ^ (roc >> 16); iv[2] = key->salt[2] ^ (roc << 16) ^ seq;
}
// the tag over (aad || word, ct) under the key whose table is tab
SX_HD void sx_gcm_tag(const SxSrtpKey* key, const u32* te, const u32* iv, const u32* tab, int stride, const u32* red, const u8* aad, i32 n_aad, u32 word, i32 n_word,
                      const u8* ct, i32 n_ct, u32* tag) {
    u32 y[4];
    sx_gcm_ghash(tab, stride, red, aad, n_aad, word, n_word, ct, n_ct, y);
    sx_aes_block(key->rk, te, iv[0], iv[1], iv[2], 1u, tag);
#pragma unroll
    for (int k = 0; k < 4; k++) tag[k] ^= y[k];
}
SX_HD void sx_gcm_put_tag(u8* q, const u32* tag) {
#pragma unroll
    for (int b = 0; b < SX_GCM_TAG; b++) q[b] = (u8)(tag[b >> 2] >> (8 * (3 - (b & 3))));
}
// tag[0 .. 4) against the 16 bytes at q, read inside [lo, hi): 0 = equal
SX_HD u32 sx_gcm_tag_diff(const u32* tag, const u8* q, const u8* lo, const u8* hi) {
    u32 diff = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) diff |= tag[k] ^ sx_rtp_be32(q + 4 * k, lo, hi);
    return diff;
}
// the cipher over one datagram: p[from .. len) ^= keystream, by `nlanes` lanes, this one being `lane` (the XOR of sx_srtp_cipher under GCM's counter)
SX_HD void sx_gcm_cipher(u8* p, i32 from, i32 len, const SxSrtpKey* key, const u32* te, u32 ssrc, u32 roc, u32 seq, int lane, int nlanes) {
    u32 iv[3];
    sx_gcm_iv(key, ssrc, roc, seq, iv);
    const i32 n = len - from, n_blocks = (n + 15) >> 4;
    u8* q = p + from;
    const bool aligned = ((uintptr_t)q & 3) == 0;
    for (i32 j = lane; j < n_blocks; j += nlanes) {
        u32 ks[4];
        sx_aes_block(key->rk, te, iv[0], iv[1], iv[2], (u32)j + 2u, ks);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const i32 at = 16 * j + 4 * k;
            if (aligned && at + 4 <= n) {
                u32* d = (u32*)(q + at);
                *d ^= sx_rtp_bswap(ks[k]);
            } else {
#pragma unroll
                for (int b = 0; b < 4; b++)
                    if (at + b < n) q[at + b] ^= (u8)(ks[k] >> (8 * (3 - b)));
            }
        }
    }
}

// ---- the control plane (host) ---------------------------------------------------------------------------------------------------------------
// one direction's 28 bytes of keying material (master key || 12-byte master salt) -> its record.  The PRF is that of RFC 3711 section 4.3
// with the salt padded on the right to 14 bytes; label: that of the cipher key (0 SRTP, 3 SRTCP), the salt's is label + 2; there is no
// authentication key.  ke / ks: where the test wants the session key and salt
static inline void sx_srtp_gcm_session_record(const u8* ke, const u8* ks, SxSrtpKey* rec) {
    memset(rec, 0, sizeof(*rec));
    sx_aes_expand(ke, rec->rk);
    for (int k = 0; k < 3; k++) rec->salt[k] = ((u32)ks[4 * k] << 24) | ((u32)ks[4 * k + 1] << 16) | ((u32)ks[4 * k + 2] << 8) | ks[4 * k + 3];
    sx_aes_block(rec->rk, SX_AES_TE0, 0, 0, 0, 0, rec->mid_i);                  // H
    rec->tag = SX_GCM_TAG; rec->has = 1; rec->transform = SX_SRTP_GCM;
}
static inline void sx_srtp_gcm_make_key_at(const u8* master, int label, SxSrtpKey* rec, u8* ke_out, u8* ks_out) {
    u32 mrk[44];
    u8 ke[16], ks[12], salt[14];
    memcpy(salt, master + 16, 12);
    salt[12] = salt[13] = 0;
    sx_aes_expand(master, mrk);
    sx_srtp_prf(mrk, salt, label, ke, 16);
    sx_srtp_prf(mrk, salt, label + 2, ks, 12);
    sx_srtp_gcm_session_record(ke, ks, rec);
    if (ke_out) memcpy(ke_out, ke, 16);
    if (ks_out) memcpy(ks_out, ks, 12);
    volatile u8* z = ke;
    for (int k = 0; k < 16; k++) z[k] = 0;
    volatile u32* zr = mrk;
    for (int k = 0; k < 44; k++) zr[k] = 0;
}
// solo_srtp_set_keys_gcm: sx_srtp_set_keys_plan with 28-byte masters and the one tag
static inline bool sx_srtp_gcm_set_keys_plan(const SxSrtpMirror& m, int32_t n_streams, int32_t trailer, const int32_t* streams, int32_t n, const u8* tx_master,
                                             const u8* rx_master, const u32* rx_roc, SxSrtpMirror& next, std::vector<SxSrtpKey>& recs, std::vector<SxSrtpRx>& rx) {
    if (!sx_list_ok(streams, n, n_streams) || (!tx_master && !rx_master) || (tx_master && trailer < SX_GCM_TAG)) return false;
    next = m;
    next.tx_tag.resize((size_t)n_streams, 0); next.rx_tag.resize((size_t)n_streams, 0);
    recs.resize(2 * (size_t)n); rx.resize((size_t)n);
    for (int32_t i = 0; i < n; i++) {
        memset(&recs[2 * (size_t)i], 0, 2 * sizeof(SxSrtpKey));
        if (tx_master) { sx_srtp_gcm_make_key_at(tx_master + SX_GCM_MASTER * (size_t)i, 0, &recs[2 * (size_t)i], NULL, NULL); next.tx_tag[(size_t)streams[i]] = SX_GCM_TAG; }
        if (rx_master) { sx_srtp_gcm_make_key_at(rx_master + SX_GCM_MASTER * (size_t)i, 0, &recs[2 * (size_t)i + 1], NULL, NULL); next.rx_tag[(size_t)streams[i]] = SX_GCM_TAG; }
        SxSrtpRx x; x.index = -1; x.pending = 0; x.roc0 = rx_roc ? rx_roc[i] : 0u; x.pad[0] = x.pad[1] = x.pad[2] = 0;
        rx[(size_t)i] = x;
    }
    return true;
}
// the SRTP mirror holds tag lengths, and 16 is only GCM's: the streams that hold a GCM key in this direction (counted when the mirror
// changes, never by a device call)
static inline int32_t sx_srtp_gcm_count(const std::vector<u8>& tags) {
    int32_t n = 0;
    for (size_t s = 0; s < tags.size(); s++) n += tags[s] == SX_GCM_TAG;
    return n;
}
// the SRTCP mirror's "has tx / has rx" byte: 1 under the HMAC transform, SX_SRTCP_HAS_GCM under this one
#define SX_SRTCP_HAS_GCM 2
static inline bool sx_srtcp_gcm_set_keys_plan(const SxSrtcpMirror& m, int32_t n_streams, const int32_t* streams, int32_t n, const u8* tx_master, const u8* rx_master,
                                              const u32* tx_index, const i64* rx_index, SxSrtcpMirror& next, std::vector<SxSrtpKey>& recs, std::vector<SxSrtcpTx>& tx,
                                              std::vector<SxSrtcpRx>& rx) {
    if (!sx_list_ok(streams, n, n_streams) || (!tx_master && !rx_master)) return false;
    for (int32_t i = 0; i < n; i++)
        if ((tx_index && tx_index[i] > SX_SRTCP_INDEX_END) || (rx_index && (rx_index[i] < -1 || rx_index[i] >= (i64)SX_SRTCP_INDEX_END))) return false;
    next = m;
    next.has_tx.resize((size_t)n_streams, 0); next.has_rx.resize((size_t)n_streams, 0);
    recs.resize(2 * (size_t)n); tx.resize((size_t)n); rx.resize((size_t)n);
    for (int32_t i = 0; i < n; i++) {
        memset(&recs[2 * (size_t)i], 0, 2 * sizeof(SxSrtpKey));
        if (tx_master) { sx_srtp_gcm_make_key_at(tx_master + SX_GCM_MASTER * (size_t)i, 3, &recs[2 * (size_t)i], NULL, NULL); next.has_tx[(size_t)streams[i]] = SX_SRTCP_HAS_GCM; }
        if (rx_master) { sx_srtp_gcm_make_key_at(rx_master + SX_GCM_MASTER * (size_t)i, 3, &recs[2 * (size_t)i + 1], NULL, NULL); next.has_rx[(size_t)streams[i]] = SX_SRTCP_HAS_GCM; }
        tx[(size_t)i].next = tx_index ? tx_index[i] : 0u;
        rx[(size_t)i].index = rx_index ? rx_index[i] : -1; rx[(size_t)i].pending = 0;
    }
    return true;
}
static inline int32_t sx_srtcp_gcm_count(const std::vector<u8>& has) {
    int32_t n = 0;
    for (size_t s = 0; s < has.size(); s++) n += has[s] == SX_SRTCP_HAS_GCM;
    return n;
}
// solo_srtcp_protect: a session that holds a GCM tx key needs the longer trailer behind every packet of the build call
static inline bool sx_srtcp_gcm_protect_ok(bool any_gcm_tx, int trailer) { return trailer >= SX_SRTCP_GCM_TRAILER || !any_gcm_tx; }

// ---- SRTP ---------------------------------------------------------------------------------------------------------------------------------
// THE send rule of sx_srtp_protect_plan for the datagrams it left: those whose record names a stream under a GCM tx key
SX_HD i32 sx_srtp_gcm_protect_plan(const SxSrtpProtectArgs& a, int k, SxSrtpRun* run) {
    const SxRtpDgram d = a.dgrams[k];
    sx_srtcp_run_clear(run);
    const SxSendRecord r = a.records[k];
    if (d.len == 0 || !a.keys || r.stream < 0 || r.stream >= a.n_streams || sx_srtp_key(a.keys, r.stream, 0)->transform != SX_SRTP_GCM) return run->verdict = SX_SRTP_ELSEWHERE;
    const SxRtpDgram none = {0, 0};
    a.dgrams[k] = none;                                     // (written again behind the tag)
    if (d.len < 12 || d.offset < 0 || (i64)d.offset + (i64)d.len > a.wire_bytes || r.seq < 0 || r.desc < 0 || r.desc > 1) return run->verdict = SX_SRTP_MALFORMED;
    SxRtpHead hd;
    const i32 hdr = sx_rtp_header_walk(a.wire + d.offset, d.len, &hd);
    if (hdr < 0 || (i64)d.offset + (i64)d.len + SX_GCM_TAG > a.wire_bytes) return run->verdict = SX_SRTP_MALFORMED;
    const SxRtpStream c = a.cfg[r.stream];
    const i64 index = (i64)(c.seq_pt & 0xFFFFu) + 2 * (i64)r.seq + (i64)r.desc;
    run->off = d.offset; run->len = d.len; run->hdr = hdr; run->stream = r.stream;
    run->roc = (u32)(index >> 16); run->seq = (u32)index & 0xFFFFu; run->ssrc = c.ssrc;
    return run->verdict = SX_SRTP_OK;
}
// the tag behind the ciphertext, and the datagram's entry with the tag counted in
SX_HD void sx_srtp_gcm_protect_tag(const SxSrtpProtectArgs& a, int k, const SxSrtpRun& r, const u32* te, const u32* tab, int stride, const u32* red) {
    const SxSrtpKey* key = sx_srtp_key(a.keys, r.stream, 0);
    u8* p = a.wire + r.off;
    u32 iv[3], tag[4];
    sx_gcm_iv(key, r.ssrc, r.roc, r.seq, iv);
    sx_gcm_tag(key, te, iv, tab, stride, red, p, r.hdr, 0u, 0, p + r.hdr, r.len - r.hdr, tag);
    sx_gcm_put_tag(p + r.len, tag);
    SxRtpDgram d; d.offset = r.off; d.len = r.len + SX_GCM_TAG;
    a.dgrams[k] = d;
}
// THE receive rule of sx_srtp_unprotect_one for the datagrams it left (those of a stream under a GCM rx key; it has written d_dgrams_out[i]
// back to what came in): malformed with T = 16, then the estimate, the tag, the pending index.  tab: this lane's table, built here
SX_HD i32 sx_srtp_gcm_unprotect_one(const SxSrtpUnprotectArgs& a, int i, SxSrtpRun* run, const u32* te, u32* tab, int stride, const u32* red) {
    const SxRtpDgram d = a.dgrams[i];
    sx_srtcp_run_clear(run);
    if (d.len < 12 + SX_SRTP_MIN_TAG || d.offset < 0 || (i64)d.offset + (i64)d.len > a.wire_bytes || !a.keys || !a.rx) return run->verdict = SX_SRTP_ELSEWHERE;
    const u8* lo = a.wire + d.offset;
    const u8* hi = lo + d.len;
    const u32 ssrc = sx_rtp_be32(lo + 8, lo, hi);
    const i32 stream = sx_rtp_find_ssrc(a.table, ssrc);
    if (stream < 0 || stream >= a.n_streams) return run->verdict = SX_SRTP_ELSEWHERE;
    const SxSrtpKey* key = sx_srtp_key(a.keys, stream, 1);
    if (!key->has || key->transform != SX_SRTP_GCM) return run->verdict = SX_SRTP_ELSEWHERE;
    const SxRtpDgram none = {0, 0};
    a.out[i] = none;
    SxRtpHead hd;
    const i32 body = d.len - SX_GCM_TAG;                     // header and ciphertext
    const i32 hdr = body < 12 ? -1 : sx_rtp_header_walk(lo, body, &hd);
    if (hdr < 0) return run->verdict = SX_SRTP_MALFORMED;
    const u32 seq = hd.w0 & 0xFFFFu;
    const i64 index = sx_srtp_guess_index(a.rx[stream], seq);
    u32 iv[3], tag[4];
    sx_gcm_table(key->mid_i, tab, stride);
    sx_gcm_iv(key, ssrc, (u32)(index >> 16), seq, iv);
    sx_gcm_tag(key, te, iv, tab, stride, red, lo, hdr, 0u, 0, lo + hdr, body - hdr, tag);
    if (sx_gcm_tag_diff(tag, lo + body, lo, hi)) return run->verdict = SX_SRTP_AUTH_FAILED;
    run->off = d.offset; run->len = body; run->hdr = hdr; run->stream = stream;
    run->roc = (u32)(index >> 16); run->seq = seq; run->ssrc = ssrc;
    SxRtpDgram o; o.offset = d.offset; o.len = body;
    a.out[i] = o;
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMax((unsigned long long*)&a.rx[stream].pending, (unsigned long long)(index + 1));
#else
    if ((u64)(index + 1) > a.rx[stream].pending) a.rx[stream].pending = (u64)(index + 1);
#endif
    return run->verdict = SX_SRTP_OK;
}

// ---- SRTCP --------------------------------------------------------------------------------------------------------------------------------
// THE send rule of sx_srtcp_protect_plan for the datagrams it left
SX_HD i32 sx_srtcp_gcm_protect_plan(const SxSrtcpProtectArgs& a, int i, SxSrtpRun* run) {
    const SxRtpDgram d = a.dgrams[i];
    sx_srtcp_run_clear(run);
    const i32 s = a.streams[i];
    if (d.len == 0 || !a.keys || s < 0 || s >= a.n_streams || sx_srtp_key(a.keys, s, 0)->transform != SX_SRTP_GCM) return run->verdict = SX_SRTCP_ELSEWHERE;
    const SxRtpDgram none = {0, 0};
    a.dgrams[i] = none;                                     // (written again behind the tag)
    if (d.len < SX_SRTCP_HEAD || (d.len & 3) || d.offset < 0 || (i64)d.offset + (i64)d.len + SX_SRTCP_GCM_TRAILER > a.wire_bytes) return run->verdict = SX_SRTP_MALFORMED;
    const u32 index = a.tx[s].next;
    if (index >= SX_SRTCP_INDEX_END) return run->verdict = SX_SRTCP_EXHAUSTED;
    a.tx[s].next = index + 1u;
    const u8* lo = a.wire + d.offset;
    run->off = d.offset; run->len = d.len; run->hdr = SX_SRTCP_HEAD; run->stream = s;
    run->roc = index >> 16; run->seq = index & 0xFFFFu; run->ssrc = sx_rtp_be32(lo + 4, lo, lo + d.len);
    return run->verdict = SX_SRTP_OK;
}
// the tag behind the ciphertext, the E || index word behind the tag, and the datagram's entry with both counted in
SX_HD void sx_srtcp_gcm_protect_tag(const SxSrtcpProtectArgs& a, int i, const SxSrtpRun& r, const u32* te, const u32* tab, int stride, const u32* red) {
    const SxSrtpKey* key = sx_srtp_key(a.keys, r.stream, 0);
    const u32 word = 0x80000000u | (r.roc << 16) | r.seq;
    u8* p = a.wire + r.off;
    u32 iv[3], tag[4];
    sx_gcm_iv(key, r.ssrc, r.roc, r.seq, iv);
    sx_gcm_tag(key, te, iv, tab, stride, red, p, SX_SRTCP_HEAD, word, 4, p + SX_SRTCP_HEAD, r.len - SX_SRTCP_HEAD, tag);
    sx_gcm_put_tag(p + r.len, tag);
#pragma unroll
    for (int b = 0; b < 4; b++) p[r.len + SX_GCM_TAG + b] = (u8)(word >> (8 * (3 - b)));
    SxRtpDgram d; d.offset = r.off; d.len = r.len + SX_SRTCP_GCM_TRAILER;
    a.dgrams[i] = d;
}
// THE receive rule of sx_srtcp_unprotect_one for the datagrams it left: malformed below 8 + 20 bytes, the word in the LAST four bytes, the
// replay rule, the tag.  A run with E = 0 has hdr = len: no cipher
SX_HD i32 sx_srtcp_gcm_unprotect_one(const SxSrtcpUnprotectArgs& a, int i, SxSrtpRun* run, const u32* te, u32* tab, int stride, const u32* red) {
    const SxRtpDgram d = a.dgrams[i];
    sx_srtcp_run_clear(run);
    if (d.len < SX_SRTCP_HEAD + SX_SRTCP_TRAILER || d.offset < 0 || (i64)d.offset + (i64)d.len > a.wire_bytes || !a.keys || !a.rx) return run->verdict = SX_SRTCP_ELSEWHERE;
    const u8* lo = a.wire + d.offset;
    const u8* hi = lo + d.len;
    const u32 ssrc = sx_rtp_be32(lo + 4, lo, hi);
    const i32 stream = sx_rtp_find_ssrc(a.table, ssrc);
    if (stream < 0 || stream >= a.n_streams) return run->verdict = SX_SRTCP_ELSEWHERE;
    const SxSrtpKey* key = sx_srtp_key(a.keys, stream, 1);
    if (!key->has || key->transform != SX_SRTP_GCM) return run->verdict = SX_SRTCP_ELSEWHERE;
    const SxRtpDgram none = {0, 0};
    a.out[i] = none;
    if (d.len < SX_SRTCP_HEAD + SX_SRTCP_GCM_TRAILER) return run->verdict = SX_SRTP_MALFORMED;
    const i32 body = d.len - SX_SRTCP_GCM_TRAILER;           // the packet: what comes out
    const u32 word = sx_rtp_be32(hi - 4, lo, hi), index = word & 0x7FFFFFFFu;
    if ((i64)index <= a.rx[stream].index) return run->verdict = SX_SRTCP_REPLAYED;
    const i32 from = (word >> 31) ? SX_SRTCP_HEAD : body;    // E = 0: all of it is associated data
    u32 iv[3], tag[4];
    sx_gcm_table(key->mid_i, tab, stride);
    sx_gcm_iv(key, ssrc, index >> 16, index & 0xFFFFu, iv);
    sx_gcm_tag(key, te, iv, tab, stride, red, lo, from, word, 4, lo + from, body - from, tag);
    if (sx_gcm_tag_diff(tag, lo + body, lo, hi)) return run->verdict = SX_SRTP_AUTH_FAILED;
    run->off = d.offset; run->len = body; run->hdr = from; run->stream = stream;
    run->roc = index >> 16; run->seq = index & 0xFFFFu; run->ssrc = ssrc;
    SxRtpDgram o; o.offset = d.offset; o.len = body;
    a.out[i] = o;
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMax((unsigned long long*)&a.rx[stream].pending, (unsigned long long)index + 1ull);
#else
    if ((u64)index + 1u > a.rx[stream].pending) a.rx[stream].pending = (u64)index + 1u;
#endif
    return run->verdict = SX_SRTP_OK;
}
SX_HD void sx_gcm_run_cipher(u8* wire, const SxSrtpKey* keys, int dir, const SxSrtpRun& r, const u32* te, int lane, int nlanes) {
    sx_gcm_cipher(wire + r.off, r.hdr, r.len, sx_srtp_key(keys, r.stream, dir), te, r.ssrc, r.roc, r.seq, lane, nlanes);
}

#if defined(__HIPCC__)
// what the four kernels share: the tables and counters of a workgroup, and the row loop over the tile's accepted runs
struct SxGcmLds { u32 te[256]; u32 red[16]; i32 cnt[16]; SxSrtpRun runs[SX_GCM_TILE]; u32 tab[SX_GCM_TABLE_WORDS * SX_GCM_TILE]; };
static_assert(sizeof(SxGcmLds) <= 20 * 1024, "eight one-wave workgroups in the 160 KB of a CU's LDS");
__device__ __forceinline__ void sx_gcm_lds_init(SxGcmLds& l) {
    const int tid = (int)threadIdx.x;
#pragma unroll
    for (int j = 0; j < 256; j += SX_GCM_TILE) l.te[j + tid] = SX_AES_TE0_DEV[j + tid];
    if (tid < 16) { l.red[tid] = SX_GCM_RED_DEV[tid]; l.cnt[tid] = 0; }
    __syncthreads();
}
__device__ __forceinline__ void sx_gcm_rows(SxGcmLds& l, u8* wire, const SxSrtpKey* keys, int dir) {
    const int tid = (int)threadIdx.x, lane = tid & (SX_RTP_ROW - 1);
    for (int t = tid / SX_RTP_ROW; t < SX_GCM_TILE; t += SX_GCM_TILE / SX_RTP_ROW) {
        const SxSrtpRun r = l.runs[t];
        if (r.verdict == SX_SRTP_OK) sx_gcm_run_cipher(wire, keys, dir, r, l.te, lane, SX_RTP_ROW);
    }
}
// Each runs behind the kernel of solo_srtp.h / solo_srtcp.h with the same arguments and adds to the count that kernel wrote
__global__ void __launch_bounds__(SX_GCM_TILE) solo_srtp_gcm_protect_kernel(const SxSrtpProtectArgs a, i32* count) {
    __shared__ SxGcmLds l;
    const i32 n = sx_srtp_n_records(a);
    if (n < 0) return;                                      // (refused: the kernel in front has said so)
    const int tid = (int)threadIdx.x;
    const int k = (int)blockIdx.x * SX_GCM_TILE + tid;
    sx_gcm_lds_init(l);
    SxSrtpRun run;
    sx_srtcp_run_clear(&run); run.verdict = -1;
    if (k < n) atomicAdd(&l.cnt[sx_srtp_gcm_protect_plan(a, k, &run)], 1);
    l.runs[tid] = run;
    if (run.verdict == SX_SRTP_OK) sx_gcm_table(sx_srtp_key(a.keys, run.stream, 0)->mid_i, l.tab + tid, SX_GCM_TILE);
    __syncthreads();
    sx_gcm_rows(l, a.wire, a.keys, 0);
    __syncthreads();                                        // (the ciphertext of this tile is written: GHASH reads it)
    if (run.verdict == SX_SRTP_OK) sx_srtp_gcm_protect_tag(a, k, run, l.te, l.tab + tid, SX_GCM_TILE, l.red);
    sx_srtp_count_flush(l.cnt, count);
}
__global__ void __launch_bounds__(SX_GCM_TILE) solo_srtp_gcm_unprotect_kernel(const SxSrtpUnprotectArgs a, i32* count) {
    __shared__ SxGcmLds l;
    const int tid = (int)threadIdx.x;
    const int i = (int)blockIdx.x * SX_GCM_TILE + tid;
    sx_gcm_lds_init(l);
    SxSrtpRun run;
    sx_srtcp_run_clear(&run); run.verdict = -1;
    if (i < a.n_dgrams) atomicAdd(&l.cnt[sx_srtp_gcm_unprotect_one(a, i, &run, l.te, l.tab + tid, SX_GCM_TILE, l.red)], 1);
    l.runs[tid] = run;
    __syncthreads();
    sx_gcm_rows(l, a.wire, a.keys, 1);
    sx_srtp_count_flush(l.cnt, count);
}
__global__ void __launch_bounds__(SX_GCM_TILE) solo_srtcp_gcm_protect_kernel(const SxSrtcpProtectArgs a, i32* count) {
    __shared__ SxGcmLds l;
    if (sx_srtcp_refused(a)) return;                        // (the kernel in front has said so)
    const int tid = (int)threadIdx.x;
    const int i = (int)blockIdx.x * SX_GCM_TILE + tid;
    sx_gcm_lds_init(l);
    SxSrtpRun run;
    sx_srtcp_run_clear(&run); run.verdict = -1;
    if (i < a.n) atomicAdd(&l.cnt[sx_srtcp_gcm_protect_plan(a, i, &run)], 1);
    l.runs[tid] = run;
    if (run.verdict == SX_SRTP_OK) sx_gcm_table(sx_srtp_key(a.keys, run.stream, 0)->mid_i, l.tab + tid, SX_GCM_TILE);
    __syncthreads();
    sx_gcm_rows(l, a.wire, a.keys, 0);
    __syncthreads();                                        // (the ciphertext of this tile is written: GHASH reads it)
    if (run.verdict == SX_SRTP_OK) sx_srtcp_gcm_protect_tag(a, i, run, l.te, l.tab + tid, SX_GCM_TILE, l.red);
    sx_srtcp_count_flush(l.cnt, count);
}
__global__ void __launch_bounds__(SX_GCM_TILE) solo_srtcp_gcm_unprotect_kernel(const SxSrtcpUnprotectArgs a, i32* count) {
    __shared__ SxGcmLds l;
    const int tid = (int)threadIdx.x;
    const int i = (int)blockIdx.x * SX_GCM_TILE + tid;
    sx_gcm_lds_init(l);
    SxSrtpRun run;
    sx_srtcp_run_clear(&run); run.verdict = -1;
    if (i < a.n_dgrams) atomicAdd(&l.cnt[sx_srtcp_gcm_unprotect_one(a, i, &run, l.te, l.tab + tid, SX_GCM_TILE, l.red)], 1);
    l.runs[tid] = run;
    __syncthreads();
    sx_gcm_rows(l, a.wire, a.keys, 1);
    sx_srtcp_count_flush(l.cnt, count);
}
// The launches of the four calls.  gcm: the host mirror holds a GCM key in the call's direction; without one the call enqueues exactly
// what solo_srtp.h / solo_srtcp.h enqueue.  The fold kernels stay last
static inline hipError_t solo_srtp_protect_launch_all(const SxSrtpProtectArgs& a0, SxSrtpCount* count, bool gcm, hipStream_t s) {
    SxSrtpProtectArgs a = a0;
    a.gcm = gcm ? 1 : 0;
    const hipError_t e = solo_srtp_protect_launch(a, count, s);
    if (!gcm || e != hipSuccess) return e;
    hipLaunchKernelGGL(solo_srtp_gcm_protect_kernel, dim3((a.max_records + SX_GCM_TILE - 1) / SX_GCM_TILE), dim3(SX_GCM_TILE), 0, s, a, (i32*)count);
    return hipGetLastError();
}
static inline hipError_t solo_srtp_unprotect_launch_all(const SxSrtpUnprotectArgs& a0, SxSrtpCount* count, bool gcm, hipStream_t s) {
    SxSrtpUnprotectArgs a = a0;
    a.gcm = gcm ? 1 : 0;
    hipError_t e = solo_srtp_unprotect_launch_verdicts(a, count, s);
    if (gcm && a.n_dgrams > 0 && e == hipSuccess) {
        hipLaunchKernelGGL(solo_srtp_gcm_unprotect_kernel, dim3((a.n_dgrams + SX_GCM_TILE - 1) / SX_GCM_TILE), dim3(SX_GCM_TILE), 0, s, a, (i32*)count);
        e = hipGetLastError();
    }
    return e != hipSuccess ? e : solo_srtp_unprotect_launch_fold(a, s);
}
static inline hipError_t solo_srtcp_protect_launch_all(const SxSrtcpProtectArgs& a0, SxSrtcpCount* count, bool gcm, hipStream_t s) {
    SxSrtcpProtectArgs a = a0;
    a.gcm = gcm ? 1 : 0;
    const hipError_t e = solo_srtcp_protect_launch(a, count, s);
    if (!gcm || e != hipSuccess) return e;
    hipLaunchKernelGGL(solo_srtcp_gcm_protect_kernel, dim3((a.n + SX_GCM_TILE - 1) / SX_GCM_TILE), dim3(SX_GCM_TILE), 0, s, a, (i32*)count);
    return hipGetLastError();
}
static inline hipError_t solo_srtcp_unprotect_launch_all(const SxSrtcpUnprotectArgs& a0, SxSrtcpCount* count, bool gcm, hipStream_t s) {
    SxSrtcpUnprotectArgs a = a0;
    a.gcm = gcm ? 1 : 0;
    hipError_t e = solo_srtcp_unprotect_launch_verdicts(a, count, s);
    if (gcm && a.n_dgrams > 0 && e == hipSuccess) {
        hipLaunchKernelGGL(solo_srtcp_gcm_unprotect_kernel, dim3((a.n_dgrams + SX_GCM_TILE - 1) / SX_GCM_TILE), dim3(SX_GCM_TILE), 0, s, a, (i32*)count);
        e = hipGetLastError();
    }
    return e != hipSuccess ? e : solo_srtcp_unprotect_launch_fold(a, s);
}
#else
// Host forms (tests): the GCM kernels' work behind sx_srtp_*_host / sx_srtcp_*_host, adding to the count those wrote; tile by tile, phase
// by phase, lane by lane through the per-datagram functions above.  A lane's table is 64 words of its own (stride 1).
template <typename Args, typename Plan, typename Tag>
static inline void sx_gcm_protect_host(const Args& a, i32 n, i32* count, int n_counted, Plan plan, Tag tag) {
    i32 c[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    SxSrtpRun* runs = new SxSrtpRun[SX_GCM_TILE];
    u32* tab = new u32[SX_GCM_TABLE_WORDS * SX_GCM_TILE];
    for (int t0 = 0; t0 < n; t0 += SX_GCM_TILE) {
        const int m = sx_min(n - t0, SX_GCM_TILE);
        for (int t = 0; t < m; t++) {
            c[plan(a, t0 + t, &runs[t])]++;
            if (runs[t].verdict == SX_SRTP_OK) sx_gcm_table(sx_srtp_key(a.keys, runs[t].stream, 0)->mid_i, tab + t, SX_GCM_TILE);
        }
        for (int t = 0; t < m; t++)
            for (int lane = 0; lane < SX_RTP_ROW && runs[t].verdict == SX_SRTP_OK; lane++) sx_gcm_run_cipher(a.wire, a.keys, 0, runs[t], SX_AES_TE0, lane, SX_RTP_ROW);
        for (int t = 0; t < m; t++)
            if (runs[t].verdict == SX_SRTP_OK) tag(a, t0 + t, runs[t], SX_AES_TE0, tab + t, SX_GCM_TILE, SX_GCM_RED);
    }
    delete[] runs;
    delete[] tab;
    for (int k = 0; k < n_counted; k++) count[k] += c[k];
}
template <typename Args, typename One>
static inline void sx_gcm_unprotect_host(const Args& a, i32* count, int n_counted, One one) {
    i32 c[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    SxSrtpRun* runs = new SxSrtpRun[SX_GCM_TILE];
    u32* tab = new u32[SX_GCM_TABLE_WORDS * SX_GCM_TILE];
    for (int t0 = 0; t0 < a.n_dgrams; t0 += SX_GCM_TILE) {
        const int m = sx_min(a.n_dgrams - t0, SX_GCM_TILE);
        for (int t = 0; t < m; t++) c[one(a, t0 + t, &runs[t], SX_AES_TE0, tab + t, SX_GCM_TILE, SX_GCM_RED)]++;
        for (int t = 0; t < m; t++)
            for (int lane = 0; lane < SX_RTP_ROW && runs[t].verdict == SX_SRTP_OK; lane++) sx_gcm_run_cipher(a.wire, a.keys, 1, runs[t], SX_AES_TE0, lane, SX_RTP_ROW);
    }
    delete[] runs;
    delete[] tab;
    for (int k = 0; k < n_counted; k++) count[k] += c[k];
}
// the four calls as solo_api.hip issues them: the older transform's pass, this one's, the fold last
static inline void sx_srtp_protect_host_all(const SxSrtpProtectArgs& a0, SxSrtpCount* count) {
    SxSrtpProtectArgs a = a0;
    a.gcm = 1;
    sx_srtp_protect_host(a, count);
    if (sx_srtp_n_records(a) >= 0) sx_gcm_protect_host(a, sx_srtp_n_records(a), (i32*)count, 6, sx_srtp_gcm_protect_plan, sx_srtp_gcm_protect_tag);
}
static inline void sx_srtp_unprotect_host_all(const SxSrtpUnprotectArgs& a0, SxSrtpCount* count) {
    SxSrtpUnprotectArgs a = a0;
    a.gcm = 1;
    sx_srtp_unprotect_host(a, count);                       // (its fold finds nothing pending of this transform's yet)
    sx_gcm_unprotect_host(a, (i32*)count, 6, sx_srtp_gcm_unprotect_one);
    if (a.rx)
        for (int s = 0; s < a.n_streams; s++) sx_srtp_rx_fold(a.rx, s);
}
static inline void sx_srtcp_protect_host_all(const SxSrtcpProtectArgs& a0, SxSrtcpCount* count) {
    SxSrtcpProtectArgs a = a0;
    a.gcm = 1;
    sx_srtcp_protect_host(a, count);
    if (!sx_srtcp_refused(a)) sx_gcm_protect_host(a, a.n, (i32*)count, 8, sx_srtcp_gcm_protect_plan, sx_srtcp_gcm_protect_tag);
}
static inline void sx_srtcp_unprotect_host_all(const SxSrtcpUnprotectArgs& a0, SxSrtcpCount* count) {
    SxSrtcpUnprotectArgs a = a0;
    a.gcm = 1;
    sx_srtcp_unprotect_host(a, count);
    sx_gcm_unprotect_host(a, (i32*)count, 8, sx_srtcp_gcm_unprotect_one);
    if (a.rx)
        for (int s = 0; s < a.n_streams; s++) sx_srtp_rx_fold(a.rx, s);
}
#endif

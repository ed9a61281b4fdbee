// solo_srtp.h -- SRTP (RFC 3711) with the mandatory default transforms as a stage of the RTP session (solo_srtp_protect behind
// solo_rtp_pack, solo_srtp_unprotect in front of solo_rtp_parse; include/solo_mi355x.h): AES-128 in counter mode over everything behind
// the RTP header, HMAC-SHA1 over header, ciphertext and rollover counter with an 80- or 32-bit tag, the key derivation of section 4.3
// with rate 0.  Both calls work in place on the wire buffer.
//
// A stream has one 256-byte key record per direction (SxSrtpKey: the expanded round keys, the salt at its place in the IV, the SHA-1
// states behind the HMAC's ipad and opad blocks, tag length, "has key") and one receive record (SxSrtpRx: the highest authenticated
// packet index, the initial rollover counter).  The records are made ON THE HOST by solo_srtp_set_keys (sx_srtp_make_key below) with the
// same AES block function and SHA-1 compression the kernels run.
//
// Protect is a pure function like pack: the packet index is i = seq_offset + 2 seq + desc, the unreduced integer behind pack's 16-bit
// sequence number, so ROC = (i >> 16) mod 2^32 and the sender keeps no state.
//
// Unprotect authenticates first and decrypts only what it accepted; a rejected datagram keeps every wire byte.  The rollover counter
// is estimated (RFC 3711 section 3.3.1, appendix A) against the stream's receive record AS IT STOOD WHEN THE CALL BEGAN: the verdict
// kernel only reads `index` and raises `pending` (64-bit atomicMax), a second short kernel, a lane per stream, folds pending into index.
// The result does not depend on lane or workgroup order and equals the RFC's packet-by-packet update -- unless one call holds datagrams
// of one stream MORE THAN 2^15 SEQUENCE NUMBERS APART, where the sequential receiver would have moved its estimate inside the call
// (and until a stream's first accepted datagram every datagram of a call is judged with the initial counter).
// There is NO REPLAY LIST: a replayed datagram authenticates again and reaches the ring, which drops it as `duplicate` or `late`.
//
// The cut: one workgroup per tile of SX_RTP_TILE datagrams, as in solo_rtp_scatter_kernel.  The AES table (1 KB: Te0; Te1 .. Te3 are
// rotations of it and the S-box is its second byte) is copied to LDS once per workgroup.
//     protect    plan (a lane per datagram) | barrier | cipher (a 16-lane row per datagram, a lane takes keystream blocks lane, lane + 16,
//                ...) | barrier | MAC (a lane per datagram over the ciphertext), tag, d_dgrams
//     unprotect  plan and MAC and compare (a lane per datagram) | barrier | cipher for the accepted datagrams
// The SHA-1 schedule (16 words) and the AES state stay in registers: every loop over them is unrolled to constant indices.  Loads of
// the receive side are clipped to the datagram (sx_rtp_be32 / sx_send_ld_clipped); the keystream is XORed dword-wise where the wire
// address is 4-byte aligned (always, behind pack) and byte-wise otherwise.
//
// Everything below compiles for the host as well (tests/test_srtp_model.py): the host forms run the same per-datagram functions lane
// by lane.
#pragma once
#include "solo_rtp.h"

#define SOLO_SRTP_KEY_WORDS 64
#define SX_SRTP_MIN_TAG 4       // the tag assumed for the `malformed` rule where a datagram's stream, or its key, is not known

// what became of a datagram == its word of solo_srtp_count_t
#define SX_SRTP_OK 0
#define SX_SRTP_SKIPPED 1
#define SX_SRTP_MALFORMED 2
#define SX_SRTP_UNKNOWN_SSRC 3
#define SX_SRTP_NO_KEY 4
#define SX_SRTP_AUTH_FAILED 5
// a datagram whose key names another transform (solo_srtp_gcm.h) is left as it is and counted by that transform's kernel: this word of
// the workgroup's counters is never flushed.  ONLY where the call's arguments say that this kernel follows (`gcm`, set at launch from the
// host mirror): a call issued -- or a graph captured -- before the session held such a key has no kernel behind it that could take the
// datagram, and judges it no_key, so that it is voided on the way out and rejected on the way in: the hand-over fails closed
#define SX_SRTP_ELSEWHERE 6
#define SX_SRTP_CM 0            // SxSrtpKey.transform: AES-CM with HMAC-SHA1, the records made here
#define SX_SRTP_GCM 1           //                      AEAD_AES_128_GCM (RFC 7714), the records of solo_srtp_gcm.h

typedef solo_srtp_count_t SxSrtpCount;
static_assert(sizeof(SxSrtpCount) == 32, "solo_srtp_count_t layout");

struct SxSrtpKey { u32 rk[44], salt[4], mid_i[5], mid_o[5], tag, has, transform, pad[3]; };   // big-endian words throughout
static_assert(sizeof(SxSrtpKey) == 4 * SOLO_SRTP_KEY_WORDS && sizeof(SxSrtpKey) == 256, "a key record");
struct SxSrtpRx { i64 index; u64 pending; u32 roc0, pad[3]; };   // index: -1 = none yet; pending: 1 + the call's highest accepted index, 0 = none
static_assert(sizeof(SxSrtpRx) == 32, "a receive record");

static const u32 SX_AES_TE0[256] = {                        // the host's copy (key schedule, derivation, host forms)
#include "solo_srtp_tables.inc"
};
#if defined(__HIPCC__)
__device__ static const u32 SX_AES_TE0_DEV[256] = {         // the kernels' copy, which they move to LDS
#include "solo_srtp_tables.inc"
};
#endif

SX_HD u32 sx_srtp_ror(u32 v, int n) { return (v >> n) | (v << (32 - n)); }
SX_HD u32 sx_srtp_rol(u32 v, int n) { return (v << n) | (v >> (32 - n)); }

// ---- AES-128, one block: the state is four big-endian words; te = Te0 (in LDS on the device) ---------------------------------------------
SX_HD void sx_aes_block(const u32* rk, const u32* te, u32 s0, u32 s1, u32 s2, u32 s3, u32* out) {
    s0 ^= rk[0]; s1 ^= rk[1]; s2 ^= rk[2]; s3 ^= rk[3];
#pragma unroll
    for (int r = 1; r < 10; r++) {
        const u32 t0 = te[s0 >> 24] ^ sx_srtp_ror(te[(s1 >> 16) & 255u], 8) ^ sx_srtp_ror(te[(s2 >> 8) & 255u], 16) ^ sx_srtp_ror(te[s3 & 255u], 24) ^ rk[4 * r + 0];
        const u32 t1 = te[s1 >> 24] ^ sx_srtp_ror(te[(s2 >> 16) & 255u], 8) ^ sx_srtp_ror(te[(s3 >> 8) & 255u], 16) ^ sx_srtp_ror(te[s0 & 255u], 24) ^ rk[4 * r + 1];
        const u32 t2 = te[s2 >> 24] ^ sx_srtp_ror(te[(s3 >> 16) & 255u], 8) ^ sx_srtp_ror(te[(s0 >> 8) & 255u], 16) ^ sx_srtp_ror(te[s1 & 255u], 24) ^ rk[4 * r + 2];
        const u32 t3 = te[s3 >> 24] ^ sx_srtp_ror(te[(s0 >> 16) & 255u], 8) ^ sx_srtp_ror(te[(s1 >> 8) & 255u], 16) ^ sx_srtp_ror(te[s2 & 255u], 24) ^ rk[4 * r + 3];
        s0 = t0; s1 = t1; s2 = t2; s3 = t3;
    }
#define SX_AES_S(x) ((te[(x) & 255u] >> 8) & 255u)
    out[0] = ((SX_AES_S(s0 >> 24) << 24) | (SX_AES_S(s1 >> 16) << 16) | (SX_AES_S(s2 >> 8) << 8) | SX_AES_S(s3)) ^ rk[40];
    out[1] = ((SX_AES_S(s1 >> 24) << 24) | (SX_AES_S(s2 >> 16) << 16) | (SX_AES_S(s3 >> 8) << 8) | SX_AES_S(s0)) ^ rk[41];
    out[2] = ((SX_AES_S(s2 >> 24) << 24) | (SX_AES_S(s3 >> 16) << 16) | (SX_AES_S(s0 >> 8) << 8) | SX_AES_S(s1)) ^ rk[42];
    out[3] = ((SX_AES_S(s3 >> 24) << 24) | (SX_AES_S(s0 >> 16) << 16) | (SX_AES_S(s1 >> 8) << 8) | SX_AES_S(s2)) ^ rk[43];
#undef SX_AES_S
}
// keystream block j of AES-CM: AES(k, IV + j), the sum taken over all 128 bits
SX_HD void sx_aes_cm_block(const u32* rk, const u32* te, const u32* iv, u32 j, u32* out) {
    const u32 w3 = iv[3] + j;
    u32 c = w3 < j ? 1u : 0u;
    const u32 w2 = iv[2] + c; c = (c && w2 == 0) ? 1u : 0u;
    const u32 w1 = iv[1] + c; c = (c && w1 == 0) ? 1u : 0u;
    sx_aes_block(rk, te, iv[0] + c, w1, w2, w3, out);
}

// ---- SHA-1, one compression: h += f(h, w); w[16] is the block's words and is used up as the schedule's window ----------------------------
SX_HD void sx_sha1_compress(u32* h, u32* w) {
    u32 a = h[0], b = h[1], c = h[2], d = h[3], e = h[4];
#pragma unroll
    for (int t = 0; t < 80; t++) {
        u32 wt;
        if (t < 16) wt = w[t];
        else { wt = sx_srtp_rol(w[(t + 13) & 15] ^ w[(t + 8) & 15] ^ w[(t + 2) & 15] ^ w[t & 15], 1); w[t & 15] = wt; }
        u32 f, k;
        if (t < 20) { f = (b & c) | (~b & d); k = 0x5A827999u; }
        else if (t < 40) { f = b ^ c ^ d; k = 0x6ED9EBA1u; }
        else if (t < 60) { f = (b & c) | (b & d) | (c & d); k = 0x8F1BBCDCu; }
        else { f = b ^ c ^ d; k = 0xCA62C1D6u; }
        const u32 tmp = sx_srtp_rol(a, 5) + f + e + k + wt;
        e = d; d = c; c = sx_srtp_rol(b, 30); b = a; a = tmp;
    }
    h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e;
}
// the big-endian word at byte b of  p[0 .. n) || the first n_roc bytes of roc (big-endian) || 0x80 || zeros
SX_HD u32 sx_srtp_mac_word(const u8* p, i32 n, u32 roc, i32 n_roc, i64 b) {
    if (b + 4 <= (i64)n) return sx_rtp_be32(p + b, p, p + n);
    u32 v = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const i64 at = b + k;
        u32 x = 0;
        if (at < (i64)n) x = p[at];
        else if (at < (i64)n + n_roc) x = (roc >> (8 * (3 - (int)(at - n)))) & 255u;
        else if (at == (i64)n + n_roc) x = 0x80u;
        v = (v << 8) | x;
    }
    return v;
}
// HMAC-SHA1 from its two midstates over p[0 .. n) || roc (n_roc = 4; 0: the bare message) -> the five words of the tag, by ONE lane
SX_HD void sx_srtp_mac(const u32* mid_i, const u32* mid_o, const u8* p, i32 n, u32 roc, i32 n_roc, u32* tag) {
    u32 h[5], w[16];
#pragma unroll
    for (int k = 0; k < 5; k++) h[k] = mid_i[k];
    const i64 m = (i64)n + n_roc;
    const i64 n_blocks = (m + 9 + 63) >> 6;
    const u64 bits = (u64)(64 + m) * 8u;
    for (i64 blk = 0; blk < n_blocks; blk++) {
#pragma unroll
        for (int j = 0; j < 16; j++) w[j] = sx_srtp_mac_word(p, n, roc, n_roc, 64 * blk + 4 * j);
        if (blk == n_blocks - 1) { w[14] = (u32)(bits >> 32); w[15] = (u32)bits; }
        sx_sha1_compress(h, w);
    }
#pragma unroll
    for (int k = 0; k < 5; k++) { w[k] = h[k]; tag[k] = mid_o[k]; }
    w[5] = 0x80000000u;
#pragma unroll
    for (int k = 6; k < 15; k++) w[k] = 0;
    w[15] = (64 + 20) * 8;
    sx_sha1_compress(tag, w);
}
// byte k of a tag
SX_HD u32 sx_srtp_tag_byte(const u32* tag, int k) {
    const u32 w = k < 4 ? tag[0] : k < 8 ? tag[1] : tag[2];
    return (w >> (8 * (3 - (k & 3)))) & 255u;
}

// ---- the cipher over one datagram: p[hdr .. len) ^= keystream, by `nlanes` lanes, this one being `lane` -----------------------------------
// IV = (k_s << 16) ^ (SSRC << 64) ^ (i << 16); the salt words hold k_s << 16 already
SX_HD void sx_srtp_cipher(u8* p, i32 hdr, i32 len, const SxSrtpKey* key, const u32* te, u32 ssrc, u32 roc, u32 seq, int lane, int nlanes) {
    const u32 iv[4] = {key->salt[0], key->salt[1] ^ ssrc, key->salt[2] ^ roc, key->salt[3] ^ (seq << 16)};
    const i32 n = len - hdr, n_blocks = (n + 15) >> 4;
    u8* q = p + hdr;
    const bool aligned = ((uintptr_t)q & 3) == 0;
    for (i32 j = lane; j < n_blocks; j += nlanes) {
        u32 ks[4];
        sx_aes_cm_block(key->rk, te, iv, (u32)j, ks);
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

// ---- the control plane (host): key derivation and the records -----------------------------------------------------------------------------
static inline u32 sx_aes_subword(u32 v) {
    return (((SX_AES_TE0[v >> 24] >> 8) & 255u) << 24) | (((SX_AES_TE0[(v >> 16) & 255u] >> 8) & 255u) << 16) | (((SX_AES_TE0[(v >> 8) & 255u] >> 8) & 255u) << 8) |
           ((SX_AES_TE0[v & 255u] >> 8) & 255u);
}
// FIPS-197 section 5.2: 16 key bytes -> 44 round-key words
static inline void sx_aes_expand(const u8* key, u32* rk) {
    for (int i = 0; i < 4; i++) rk[i] = ((u32)key[4 * i] << 24) | ((u32)key[4 * i + 1] << 16) | ((u32)key[4 * i + 2] << 8) | key[4 * i + 3];
    u32 rcon = 1;
    for (int i = 4; i < 44; i++) {
        u32 t = rk[i - 1];
        if ((i & 3) == 0) {
            t = sx_aes_subword((t << 8) | (t >> 24)) ^ (rcon << 24);
            rcon = (rcon << 1) ^ ((rcon & 0x80u) ? 0x11Bu : 0u);
        }
        rk[i] = rk[i - 4] ^ t;
    }
}
// RFC 3711 section 4.3.1 with key derivation rate 0 (so r = 0): n <= 32 bytes of AES-CM keystream under the master key with
// IV = (master salt ^ label << 48) << 16
static inline void sx_srtp_prf(const u32* master_rk, const u8* master_salt, int label, u8* out, int n) {
    u8 x[16];
    for (int k = 0; k < 14; k++) x[k] = master_salt[k];
    x[14] = x[15] = 0;
    x[7] ^= (u8)label;
    u32 iv[4], ks[4];
    for (int k = 0; k < 4; k++) iv[k] = ((u32)x[4 * k] << 24) | ((u32)x[4 * k + 1] << 16) | ((u32)x[4 * k + 2] << 8) | x[4 * k + 3];
    for (int at = 0; at < n; at++) {
        if ((at & 15) == 0) sx_aes_cm_block(master_rk, SX_AES_TE0, iv, (u32)(at >> 4), ks);
        out[at] = (u8)(ks[(at >> 2) & 3] >> (8 * (3 - (at & 3))));
    }
}
// the SHA-1 states behind the ipad and the opad block of HMAC under key[0 .. n), n <= 64
static inline void sx_hmac_midstates(const u8* key, int n, u32* mid_i, u32* mid_o) {
    for (int pass = 0; pass < 2; pass++) {
        u32* h = pass ? mid_o : mid_i;
        h[0] = 0x67452301u; h[1] = 0xEFCDAB89u; h[2] = 0x98BADCFEu; h[3] = 0x10325476u; h[4] = 0xC3D2E1F0u;
        u32 w[16];
        for (int j = 0; j < 16; j++) {
            u32 v = 0;
            for (int b = 0; b < 4; b++) v = (v << 8) | (u32)((4 * j + b < n ? key[4 * j + b] : 0) ^ (pass ? 0x5C : 0x36));
            w[j] = v;
        }
        sx_sha1_compress(h, w);
    }
}
// one direction's 30 bytes of keying material (master key || master salt) -> its record; ke / ks / ka: where the test wants the session keys.
// label: that of the cipher key, with the authentication key and the salt behind it (0, 1, 2 for SRTP; 3, 4, 5 for SRTCP, solo_srtcp.h)
static inline void sx_srtp_make_key_at(const u8* master, int label, int tag_bytes, SxSrtpKey* rec, u8* ke_out, u8* ks_out, u8* ka_out) {
    u32 mrk[44];
    u8 ke[16], ks[16], ka[20];
    sx_aes_expand(master, mrk);
    sx_srtp_prf(mrk, master + 16, label, ke, 16);
    sx_srtp_prf(mrk, master + 16, label + 1, ka, 20);
    sx_srtp_prf(mrk, master + 16, label + 2, ks, 14);
    ks[14] = ks[15] = 0;
    memset(rec, 0, sizeof(*rec));
    sx_aes_expand(ke, rec->rk);
    for (int k = 0; k < 4; k++) rec->salt[k] = ((u32)ks[4 * k] << 24) | ((u32)ks[4 * k + 1] << 16) | ((u32)ks[4 * k + 2] << 8) | ks[4 * k + 3];
    sx_hmac_midstates(ka, 20, rec->mid_i, rec->mid_o);
    rec->tag = (u32)tag_bytes; rec->has = 1;
    if (ke_out) memcpy(ke_out, ke, 16);
    if (ks_out) memcpy(ks_out, ks, 14);
    if (ka_out) memcpy(ka_out, ka, 20);
    volatile u8* z = ke;
    for (int k = 0; k < 16; k++) z[k] = 0;
    z = ka;
    for (int k = 0; k < 20; k++) z[k] = 0;
    volatile u32* zr = mrk;
    for (int k = 0; k < 44; k++) zr[k] = 0;
}
static inline void sx_srtp_make_key(const u8* master, int tag_bytes, SxSrtpKey* rec, u8* ke_out, u8* ks_out, u8* ka_out) {
    sx_srtp_make_key_at(master, 0, tag_bytes, rec, ke_out, ks_out, ka_out);
}

// the host mirror: per stream the tag of its tx and of its rx key (0: none) -- never the keys
struct SxSrtpMirror { std::vector<u8> tx_tag, rx_tag; };
static inline bool sx_srtp_trailer_ok(const SxSrtpMirror& m, int32_t trailer) {
    if (trailer < 0 || trailer > 16) return false;
    for (size_t s = 0; s < m.tx_tag.size(); s++)
        if ((int32_t)m.tx_tag[s] > trailer) return false;      // (a keyed sender's tag must keep its room)
    return true;
}
// A set_keys call: validated before anything changes.  true: recs[2 i + d] is the record of direction d (0 tx, 1 rx) of listed stream i
// (has = 0: that direction keeps what it had), rx[i] its new receive record where the rx key is set, next the mirror after the call
static inline bool sx_srtp_set_keys_plan(const SxSrtpMirror& m, int32_t n_streams, int32_t trailer, const int32_t* streams, int32_t n, const u8* tx_master,
                                         const u8* rx_master, const u32* rx_roc, int32_t tag_bytes, SxSrtpMirror& next, std::vector<SxSrtpKey>& recs,
                                         std::vector<SxSrtpRx>& rx) {
    if (!sx_list_ok(streams, n, n_streams) || (tag_bytes != 4 && tag_bytes != 10) || (!tx_master && !rx_master) || (tx_master && trailer < tag_bytes)) return false;
    next = m;
    next.tx_tag.resize((size_t)n_streams, 0); next.rx_tag.resize((size_t)n_streams, 0);
    recs.resize(2 * (size_t)n); rx.resize((size_t)n);
    for (int32_t i = 0; i < n; i++) {
        memset(&recs[2 * (size_t)i], 0, 2 * sizeof(SxSrtpKey));
        if (tx_master) { sx_srtp_make_key(tx_master + 30 * (size_t)i, tag_bytes, &recs[2 * (size_t)i], NULL, NULL, NULL); next.tx_tag[(size_t)streams[i]] = (u8)tag_bytes; }
        if (rx_master) { sx_srtp_make_key(rx_master + 30 * (size_t)i, tag_bytes, &recs[2 * (size_t)i + 1], NULL, NULL, NULL); next.rx_tag[(size_t)streams[i]] = (u8)tag_bytes; }
        SxSrtpRx x; x.index = -1; x.pending = 0; x.roc0 = rx_roc ? rx_roc[i] : 0u; x.pad[0] = x.pad[1] = x.pad[2] = 0;
        rx[(size_t)i] = x;
    }
    return true;
}
static inline void sx_srtp_wipe(std::vector<SxSrtpKey>& recs) {
    volatile u32* z = recs.empty() ? NULL : (volatile u32*)recs.data();
    for (size_t k = 0; k < recs.size() * SOLO_SRTP_KEY_WORDS; k++) z[k] = 0;
}

// ---- protect -----------------------------------------------------------------------------------------------------------------------------
struct SxSrtpProtectArgs {
    const SxSendRecord* records; const SxSendCount* send_count; SxRtpDgram* dgrams; u8* wire; const SxRtpStream* cfg; const SxSrtpKey* keys;   // keys: [n_streams][2] or NULL
    i64 wire_bytes;                                          // (at most 2^31 - 1)
    int max_records, n_streams;
    int gcm = 0;                                             // the GCM kernel follows this one (solo_srtp_gcm.h)
};
struct SxSrtpRun { i32 off, len, hdr, stream; u32 roc, seq, ssrc; i32 verdict; };   // one datagram of a tile: wire[off .. off + len) is what the MAC covers
static_assert(sizeof(SxSrtpRun) == 32, "a run in LDS");

SX_HD i32 sx_srtp_n_records(const SxSrtpProtectArgs& a) { return sx_min(a.send_count->records, a.max_records); }
SX_HD const SxSrtpKey* sx_srtp_key(const SxSrtpKey* keys, i32 stream, int dir) { return keys + 2 * (size_t)stream + dir; }

// THE send rule: datagram k -> its run and its verdict (OK: cipher and MAC follow); a datagram that may not leave is voided here
SX_HD i32 sx_srtp_protect_plan(const SxSrtpProtectArgs& a, int k, SxSrtpRun* run) {
    const SxRtpDgram d = a.dgrams[k];
    run->off = 0; run->len = 0; run->hdr = 0; run->stream = -1; run->roc = 0; run->seq = 0; run->ssrc = 0;
    if (d.len == 0) return run->verdict = SX_SRTP_SKIPPED;
    const SxSendRecord r = a.records[k];
    const bool other = a.keys && r.stream >= 0 && r.stream < a.n_streams && sx_srtp_key(a.keys, r.stream, 0)->transform != SX_SRTP_CM;
    if (other && a.gcm) return run->verdict = SX_SRTP_ELSEWHERE;
    const SxRtpDgram none = {0, 0};
    a.dgrams[k] = none;                                     // (written again behind the MAC)
    if (d.len < 12 || d.offset < 0 || (i64)d.offset + (i64)d.len > a.wire_bytes || r.stream < 0 || r.stream >= a.n_streams || r.seq < 0 ||
        r.desc < 0 || r.desc > 1)
        return run->verdict = SX_SRTP_MALFORMED;
    if (!a.keys || !sx_srtp_key(a.keys, r.stream, 0)->has || other) return run->verdict = SX_SRTP_NO_KEY;
    SxRtpHead hd;
    const i32 hdr = sx_rtp_header_walk(a.wire + d.offset, d.len, &hd);
    if (hdr < 0 || (i64)d.offset + (i64)d.len + (i64)sx_srtp_key(a.keys, r.stream, 0)->tag > a.wire_bytes) return run->verdict = SX_SRTP_MALFORMED;
    const SxRtpStream c = a.cfg[r.stream];
    const i64 index = (i64)(c.seq_pt & 0xFFFFu) + 2 * (i64)r.seq + (i64)r.desc;
    run->off = d.offset; run->len = d.len; run->hdr = hdr; run->stream = r.stream;
    run->roc = (u32)(index >> 16); run->seq = (u32)index & 0xFFFFu; run->ssrc = c.ssrc;
    return run->verdict = SX_SRTP_OK;
}
SX_HD void sx_srtp_protect_cipher(const SxSrtpProtectArgs& a, const SxSrtpRun& r, const u32* te, int lane, int nlanes) {
    sx_srtp_cipher(a.wire + r.off, r.hdr, r.len, sx_srtp_key(a.keys, r.stream, 0), te, r.ssrc, r.roc, r.seq, lane, nlanes);
}
// the tag behind the datagram, and the datagram's entry with the tag counted in
SX_HD void sx_srtp_protect_mac(const SxSrtpProtectArgs& a, int k, const SxSrtpRun& r) {
    const SxSrtpKey* key = sx_srtp_key(a.keys, r.stream, 0);
    u32 tag[5];
    u8* p = a.wire + r.off;
    sx_srtp_mac(key->mid_i, key->mid_o, p, r.len, r.roc, 4, tag);
    const i32 T = (i32)key->tag;
    if (T == 10) {
#pragma unroll
        for (int b = 0; b < 10; b++) p[r.len + b] = (u8)sx_srtp_tag_byte(tag, b);
    } else {
#pragma unroll
        for (int b = 0; b < 4; b++) p[r.len + b] = (u8)sx_srtp_tag_byte(tag, b);
    }
    SxRtpDgram d; d.offset = r.off; d.len = r.len + T;
    a.dgrams[k] = d;
}

// ---- unprotect ---------------------------------------------------------------------------------------------------------------------------
struct SxSrtpUnprotectArgs {
    const SxRtpDgram* dgrams; SxRtpDgram* out; u8* wire; const u32* table; const SxSrtpKey* keys; SxSrtpRx* rx;      // keys, rx: NULL = no stream has a key
    i64 wire_bytes;                                          // (at most 2^31 - 1)
    int n_dgrams, n_streams;
    int gcm = 0;                                             // the GCM kernel follows this one (solo_srtp_gcm.h)
};
// the packet index of a datagram with sequence number seq against a receive record (RFC 3711 section 3.3.1, appendix A)
SX_HD i64 sx_srtp_guess_index(const SxSrtpRx& x, u32 seq) {
    u32 v;
    if (x.index < 0) v = x.roc0;
    else {
        const u32 roc = (u32)(x.index >> 16), s_l = (u32)x.index & 0xFFFFu;
        if (s_l < 32768u) v = ((i32)seq - (i32)s_l > 32768) ? roc - 1u : roc;
        else v = ((i32)s_l - 32768 > (i32)seq) ? roc + 1u : roc;
    }
    return ((i64)v << 16) | (i64)seq;
}
// THE receive rule: datagram i -> its run and its verdict, the first rule that fails; authenticated here, by this lane.  d_dgrams_out[i]
// is written either way, and the stream's pending index is raised for an accepted datagram
SX_HD i32 sx_srtp_unprotect_one(const SxSrtpUnprotectArgs& a, int i, SxSrtpRun* run) {
    const SxRtpDgram d = a.dgrams[i];
    const SxRtpDgram none = {0, 0};
    a.out[i] = none;
    run->off = 0; run->len = 0; run->hdr = 0; run->stream = -1; run->roc = 0; run->seq = 0; run->ssrc = 0;
    if (d.len < 12 + SX_SRTP_MIN_TAG || d.offset < 0 || (i64)d.offset + (i64)d.len > a.wire_bytes) return run->verdict = SX_SRTP_MALFORMED;
    const u8* lo = a.wire + d.offset;
    const u8* hi = lo + d.len;
    const u32 ssrc = sx_rtp_be32(lo + 8, lo, hi);
    i32 stream = sx_rtp_find_ssrc(a.table, ssrc);
    if (stream >= a.n_streams) stream = -1;
    const SxSrtpKey* key = (stream >= 0 && a.keys && a.rx && sx_srtp_key(a.keys, stream, 1)->has) ? sx_srtp_key(a.keys, stream, 1) : NULL;
    if (key && key->transform != SX_SRTP_CM) {
        if (a.gcm) {                                        // the kernel behind reads dgrams[i]: where out IS dgrams the entry goes back, elsewhere out stays {0, 0}
            if (a.out == a.dgrams) a.out[i] = d;
            return run->verdict = SX_SRTP_ELSEWHERE;
        }
        key = NULL;                                         // (no kernel behind this one: no key this call can use)
    }
    const i32 T = key ? (i32)key->tag : SX_SRTP_MIN_TAG;
    SxRtpHead hd;
    const i32 body = d.len - T;                              // what the tag covers
    const i32 hdr = body < 12 ? -1 : sx_rtp_header_walk(lo, body, &hd);
    if (hdr < 0) return run->verdict = SX_SRTP_MALFORMED;
    if (stream < 0) return run->verdict = SX_SRTP_UNKNOWN_SSRC;
    if (!key) return run->verdict = SX_SRTP_NO_KEY;
    const u32 seq = hd.w0 & 0xFFFFu;
    const i64 index = sx_srtp_guess_index(a.rx[stream], seq);
    u32 tag[5];
    sx_srtp_mac(key->mid_i, key->mid_o, lo, body, (u32)(index >> 16), 4, tag);
    u32 diff = 0;
    for (int b = 0; b < T; b++) diff |= sx_srtp_tag_byte(tag, b) ^ (u32)lo[body + b];
    if (diff) return run->verdict = SX_SRTP_AUTH_FAILED;
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
SX_HD void sx_srtp_unprotect_cipher(const SxSrtpUnprotectArgs& a, const SxSrtpRun& r, const u32* te, int lane, int nlanes) {
    sx_srtp_cipher(a.wire + r.off, r.hdr, r.len, sx_srtp_key(a.keys, r.stream, 1), te, r.ssrc, r.roc, r.seq, lane, nlanes);
}
// the second kernel's lane: stream s takes the call's highest accepted index (Rx: SxSrtpRx, or the SxSrtcpRx of solo_srtcp.h)
template <typename Rx> SX_HD void sx_srtp_rx_fold(Rx* rx, int s) {
    const u64 p = rx[s].pending;
    if (p) {
        if ((i64)(p - 1) > rx[s].index) rx[s].index = (i64)(p - 1);
        rx[s].pending = 0;
    }
}

#if defined(__HIPCC__)
__device__ __forceinline__ void sx_srtp_count_flush(const i32* cnt, i32* count) {
    const int tid = (int)threadIdx.x;
    if (tid < 6 && cnt[tid]) atomicAdd(&count[tid], cnt[tid]);
}
// The count is zeroed by solo_rtp_clear_kernel ahead of this kernel (the note above that kernel says why it is no memset node)
__global__ void __launch_bounds__(SX_RTP_TILE) solo_srtp_protect_kernel(const SxSrtpProtectArgs a, i32* count) {
    __shared__ u32 te[256];
    __shared__ i32 cnt[8];
    __shared__ SxSrtpRun runs[SX_RTP_TILE];
    const i32 n = sx_srtp_n_records(a);
    if (n < 0) {
        if (blockIdx.x == 0 && threadIdx.x == 0) count[0] = -1;
        return;
    }
    const int tid = (int)threadIdx.x;
    const int k = (int)blockIdx.x * SX_RTP_TILE + tid;
    te[tid] = SX_AES_TE0_DEV[tid];
    if (tid < 8) cnt[tid] = 0;
    __syncthreads();
    SxSrtpRun run;
    run.off = 0; run.len = 0; run.hdr = 0; run.stream = -1; run.roc = 0; run.seq = 0; run.ssrc = 0; run.verdict = -1;
    if (k < n) atomicAdd(&cnt[sx_srtp_protect_plan(a, k, &run)], 1);
    runs[tid] = run;
    __syncthreads();
    const int lane = tid & (SX_RTP_ROW - 1);
    for (int t = tid / SX_RTP_ROW; t < SX_RTP_TILE; t += SX_RTP_TILE / SX_RTP_ROW) {
        const SxSrtpRun r = runs[t];
        if (r.verdict == SX_SRTP_OK) sx_srtp_protect_cipher(a, r, te, lane, SX_RTP_ROW);
    }
    __syncthreads();                                        // (the ciphertext of this tile is written: the MAC reads it)
    if (run.verdict == SX_SRTP_OK) sx_srtp_protect_mac(a, k, run);
    sx_srtp_count_flush(cnt, count);
}
__global__ void __launch_bounds__(SX_RTP_TILE) solo_srtp_unprotect_kernel(const SxSrtpUnprotectArgs a, i32* count) {
    __shared__ u32 te[256];
    __shared__ i32 cnt[8];
    __shared__ SxSrtpRun runs[SX_RTP_TILE];
    const int tid = (int)threadIdx.x;
    const int i = (int)blockIdx.x * SX_RTP_TILE + tid;
    te[tid] = SX_AES_TE0_DEV[tid];
    if (tid < 8) cnt[tid] = 0;
    __syncthreads();
    SxSrtpRun run;
    run.off = 0; run.len = 0; run.hdr = 0; run.stream = -1; run.roc = 0; run.seq = 0; run.ssrc = 0; run.verdict = -1;
    if (i < a.n_dgrams) atomicAdd(&cnt[sx_srtp_unprotect_one(a, i, &run)], 1);
    runs[tid] = run;
    __syncthreads();
    const int lane = tid & (SX_RTP_ROW - 1);
    for (int t = tid / SX_RTP_ROW; t < SX_RTP_TILE; t += SX_RTP_TILE / SX_RTP_ROW) {
        const SxSrtpRun r = runs[t];
        if (r.verdict == SX_SRTP_OK) sx_srtp_unprotect_cipher(a, r, te, lane, SX_RTP_ROW);
    }
    sx_srtp_count_flush(cnt, count);
}
__global__ void __launch_bounds__(SX_RTP_TILE) solo_srtp_rx_fold_kernel(SxSrtpRx* rx, int n_streams) {
    const int s = (int)blockIdx.x * SX_RTP_TILE + (int)threadIdx.x;
    if (s < n_streams) sx_srtp_rx_fold(rx, s);
}
static inline hipError_t solo_srtp_protect_launch(const SxSrtpProtectArgs& a, SxSrtpCount* count, hipStream_t s) {
    hipLaunchKernelGGL(solo_rtp_clear_kernel, dim3(1), dim3(64), 0, s, (i32*)count);
    hipLaunchKernelGGL(solo_srtp_protect_kernel, dim3((a.max_records + SX_RTP_TILE - 1) / SX_RTP_TILE), dim3(SX_RTP_TILE), 0, s, a, (i32*)count);
    return hipGetLastError();
}
// the two halves of an unprotect call: the clear and the verdicts, then the fold (solo_srtp_gcm.h puts its kernel between them)
static inline hipError_t solo_srtp_unprotect_launch_verdicts(const SxSrtpUnprotectArgs& a, SxSrtpCount* count, hipStream_t s) {
    hipLaunchKernelGGL(solo_rtp_clear_kernel, dim3(1), dim3(64), 0, s, (i32*)count);
    if (a.n_dgrams == 0) return hipGetLastError();
    hipLaunchKernelGGL(solo_srtp_unprotect_kernel, dim3((a.n_dgrams + SX_RTP_TILE - 1) / SX_RTP_TILE), dim3(SX_RTP_TILE), 0, s, a, (i32*)count);
    return hipGetLastError();
}
static inline hipError_t solo_srtp_unprotect_launch_fold(const SxSrtpUnprotectArgs& a, hipStream_t s) {
    if (a.n_dgrams == 0 || !a.rx) return hipSuccess;
    hipLaunchKernelGGL(solo_srtp_rx_fold_kernel, dim3((a.n_streams + SX_RTP_TILE - 1) / SX_RTP_TILE), dim3(SX_RTP_TILE), 0, s, a.rx, a.n_streams);
    return hipGetLastError();
}
static inline hipError_t solo_srtp_unprotect_launch(const SxSrtpUnprotectArgs& a, SxSrtpCount* count, hipStream_t s) {
    const hipError_t e = solo_srtp_unprotect_launch_verdicts(a, count, s);
    return e != hipSuccess ? e : solo_srtp_unprotect_launch_fold(a, s);
}
#else
// Host forms (tests): tile by tile, phase by phase, lane by lane through the per-datagram functions above.
static inline void sx_srtp_protect_host(const SxSrtpProtectArgs& a, SxSrtpCount* count) {
    i32 c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const i32 n = sx_srtp_n_records(a);
    if (n < 0) { c[0] = -1; memcpy(count, c, sizeof(*count)); return; }
    SxSrtpRun* runs = new SxSrtpRun[SX_RTP_TILE];
    for (int t0 = 0; t0 < n; t0 += SX_RTP_TILE) {
        const int m = sx_min(n - t0, SX_RTP_TILE);
        for (int t = 0; t < m; t++) c[sx_srtp_protect_plan(a, t0 + t, &runs[t])]++;
        for (int t = 0; t < m; t++)
            for (int lane = 0; lane < SX_RTP_ROW && runs[t].verdict == SX_SRTP_OK; lane++) sx_srtp_protect_cipher(a, runs[t], SX_AES_TE0, lane, SX_RTP_ROW);
        for (int t = 0; t < m; t++)
            if (runs[t].verdict == SX_SRTP_OK) sx_srtp_protect_mac(a, t0 + t, runs[t]);
    }
    delete[] runs;
    c[SX_SRTP_ELSEWHERE] = 0;
    memcpy(count, c, sizeof(*count));
}
static inline void sx_srtp_unprotect_host(const SxSrtpUnprotectArgs& a, SxSrtpCount* count) {
    i32 c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    SxSrtpRun* runs = new SxSrtpRun[SX_RTP_TILE];
    for (int t0 = 0; t0 < a.n_dgrams; t0 += SX_RTP_TILE) {
        const int m = sx_min(a.n_dgrams - t0, SX_RTP_TILE);
        for (int t = 0; t < m; t++) c[sx_srtp_unprotect_one(a, t0 + t, &runs[t])]++;
        for (int t = 0; t < m; t++)
            for (int lane = 0; lane < SX_RTP_ROW && runs[t].verdict == SX_SRTP_OK; lane++) sx_srtp_unprotect_cipher(a, runs[t], SX_AES_TE0, lane, SX_RTP_ROW);
    }
    if (a.rx)
        for (int s = 0; s < a.n_streams; s++) sx_srtp_rx_fold(a.rx, s);
    delete[] runs;
    c[SX_SRTP_ELSEWHERE] = 0;
    memcpy(count, c, sizeof(*count));
}
#endif

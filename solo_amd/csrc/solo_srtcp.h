// solo_srtcp.h -- SRTCP (RFC 3711 section 3.4) on the AES and HMAC code of solo_srtp.h: solo_srtcp_protect behind solo_rtcp_build turns the
// compound packets into SRTCP in place, solo_srtcp_unprotect in front of solo_rtcp_parse turns the peers' back (include/solo_mi355x.h has
// the rules).  An SRTCP datagram is the compound packet with its first 8 bytes (first header, sender SSRC) in the clear and the rest under
// AES-CM, then one big-endian word E << 31 | index, then the tag: always 10 bytes (HMAC_SHA1_80 also in the _32 suite), no MKI, so the
// trailer is SX_SRTCP_TRAILER = 14 bytes.  The tag covers the packet as sent and the E || index word: sx_srtp_mac with that word where
// SRTP has its rollover counter.  IV = (k_s << 16) ^ (SSRC << 64) ^ (index << 16): sx_srtp_cipher with (roc, seq) = (index >> 16,
// index & 0xFFFF) and the header's 8 bytes.
//
// Per stream the session holds, in ONE device allocation of its own made by the first solo_srtcp_set_keys (SxSrtcpMem): two key records
// (SxSrtpKey as they are, derived with labels 3 / 4 / 5 by sx_srtp_make_key_at, tag = 10), a send record {next: the index the next
// protected packet gets, 0 .. 2^31} and a receive record {index: the highest authenticated, -1 = none yet; pending}.
//
// Unlike RTP the packet carries its whole index, so nothing is estimated; and unlike RTP there is no ring behind the call to drop a
// replay, so the call has a replay rule of its own: A DATAGRAM IS ACCEPTED ONLY IF ITS INDEX IS STRICTLY NEWER THAN EVERYTHING
// AUTHENTICATED BEFORE THIS CALL.  The verdict kernel only reads `index` and raises `pending` (64-bit atomicMax); a second short kernel,
// a lane per stream, folds pending into index: the result does not depend on the order inside the call.
//
// The cut is that of solo_srtp.h: one workgroup per tile of SX_RTP_TILE datagrams, the 1 KB AES table in LDS,
//     protect    plan (a lane per datagram: verdict, the send index taken and advanced) | barrier | cipher (a 16-lane row per datagram) |
//                barrier | MAC over the ciphertext, the E || index word, the tag, d_dgrams (a lane per datagram)
//     unprotect  plan and MAC and compare (a lane per datagram) | barrier | cipher for the accepted datagrams with E = 1
// Loads of the receive side are clipped to the datagram; the keystream is XORed dword-wise where the address is 4-byte aligned (always,
// behind build) and byte-wise otherwise.  Everything below compiles for the host as well (tests/test_srtcp_model.py).
#pragma once
#include "solo_srtp.h"
#include "solo_rtcp.h"

#define SX_SRTCP_TAG 10
#define SX_SRTCP_TRAILER SOLO_SRTCP_TRAILER_BYTES
#define SX_SRTCP_HEAD 8         // bytes in the clear: the first header and the sender SSRC
#define SX_SRTCP_INDEX_END 0x80000000u      // a send record that stands here has used its key up (RFC 3711 section 9.2)

// what became of a datagram == its word of solo_srtcp_count_t; 0 .. 5 are those of solo_srtp.h
#define SX_SRTCP_REPLAYED 6
#define SX_SRTCP_EXHAUSTED 7
#define SX_SRTCP_ELSEWHERE 8    // as SX_SRTP_ELSEWHERE: the datagram is solo_srtp_gcm.h's; a word of the workgroup's counters that is never flushed

typedef solo_srtcp_count_t SxSrtcpCount;
static_assert(sizeof(SxSrtcpCount) == 32, "solo_srtcp_count_t layout");
static_assert(SX_SRTCP_TRAILER == 4 + SX_SRTCP_TAG, "E || index, then the tag");

struct SxSrtcpTx { u32 next; };
struct SxSrtcpRx { i64 index; u64 pending; };                // pending: 1 + the call's highest accepted index, 0 = none
static_assert(sizeof(SxSrtcpTx) == 4 && sizeof(SxSrtcpRx) == 16, "the send and the receive record");

// the session's SRTCP allocation: keys [n_streams][2] (tx, rx) | rx [n_streams] | tx [n_streams]
struct SxSrtcpMem { SxSrtpKey* keys; SxSrtcpRx* rx; SxSrtcpTx* tx; };
static inline size_t sx_srtcp_bytes(int n_streams) { return (size_t)n_streams * (2 * sizeof(SxSrtpKey) + sizeof(SxSrtcpRx) + sizeof(SxSrtcpTx)); }
static inline SxSrtcpMem sx_srtcp_mem(void* at, int n_streams) {
    SxSrtcpMem m = {NULL, NULL, NULL};
    if (!at) return m;                                      // (no SRTCP yet: no stream has a key)
    m.keys = (SxSrtpKey*)at; m.rx = (SxSrtcpRx*)(m.keys + 2 * (size_t)n_streams); m.tx = (SxSrtcpTx*)(m.rx + n_streams);
    return m;
}
// a fresh allocation: no key, send index 0, "none yet"
static inline void sx_srtcp_mem_init(void* at, int n_streams) {
    memset(at, 0, sx_srtcp_bytes(n_streams));
    const SxSrtcpMem m = sx_srtcp_mem(at, n_streams);
    for (int s = 0; s < n_streams; s++) m.rx[s].index = -1;
}

// ---- the control plane (host) ---------------------------------------------------------------------------------------------------------------
static inline bool sx_srtcp_trailer_ok(int32_t trailer) { return (trailer >= 0 && trailer <= 16) || trailer == 20; }        // solo_rtcp_set_trailer; 20: the GCM trailer
// the host mirror: per stream "has a tx key" and "has an rx key" -- never the keys
struct SxSrtcpMirror { std::vector<u8> has_tx, has_rx; };
// A set_keys call: validated before anything changes.  true: recs[2 i + d] is the record of direction d (0 tx, 1 rx) of listed stream i
// (has = 0: that direction keeps what it had), tx[i] / rx[i] its new send / receive record where that direction's key is set, next the
// mirror after the call
static inline bool sx_srtcp_set_keys_plan(const SxSrtcpMirror& m, int32_t n_streams, const int32_t* streams, int32_t n, const u8* tx_master, const u8* rx_master,
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
        if (tx_master) { sx_srtp_make_key_at(tx_master + 30 * (size_t)i, 3, SX_SRTCP_TAG, &recs[2 * (size_t)i], NULL, NULL, NULL); next.has_tx[(size_t)streams[i]] = 1; }
        if (rx_master) { sx_srtp_make_key_at(rx_master + 30 * (size_t)i, 3, SX_SRTCP_TAG, &recs[2 * (size_t)i + 1], NULL, NULL, NULL); next.has_rx[(size_t)streams[i]] = 1; }
        tx[(size_t)i].next = tx_index ? tx_index[i] : 0u;
        rx[(size_t)i].index = rx_index ? rx_index[i] : -1; rx[(size_t)i].pending = 0;
    }
    return true;
}

// ---- protect -----------------------------------------------------------------------------------------------------------------------------
struct SxSrtcpProtectArgs {
    const i32* streams; const SxRtcpBuildCount* build_count; SxRtpDgram* dgrams; u8* wire; const SxSrtpKey* keys; SxSrtcpTx* tx;     // keys, tx: NULL = no stream has a key
    i64 wire_bytes;                                          // (at most 2^31 - 1)
    int n, n_streams;
    int gcm = 0;                                             // the GCM kernel follows this one (solo_srtp_gcm.h): see SX_SRTP_ELSEWHERE
};
static inline bool sx_srtcp_protect_ok(const void* c, int n_streams, int trailer, const void* r, int session_streams, const void* streams, int n, const void* build_count,
                                       const void* dgrams, const void* wire, long long wire_bytes, const void* count) {
    if (!c || !r || !streams || !build_count || !dgrams || !wire || !count || session_streams != n_streams || trailer < SX_SRTCP_TRAILER) return false;
    if (n <= 0 || n > n_streams || wire_bytes < 0) return false;
    return !(((uintptr_t)streams | (uintptr_t)dgrams | (uintptr_t)wire | (uintptr_t)count) & 3) && !((uintptr_t)build_count & 7);
}
static inline bool sx_srtcp_unprotect_ok(const void* r, const void* dgrams, int n_dgrams, const void* wire, long long wire_bytes, const void* out, const void* count) {
    if (!r || n_dgrams < 0 || wire_bytes < 0 || !count || (n_dgrams > 0 && (!dgrams || !wire || !out))) return false;
    return !(((uintptr_t)dgrams | (uintptr_t)out | (uintptr_t)count) & 3);
}
SX_HD bool sx_srtcp_refused(const SxSrtcpProtectArgs& a) { return a.build_count->built < 0; }
SX_HD void sx_srtcp_run_clear(SxSrtpRun* run) { run->off = 0; run->len = 0; run->hdr = 0; run->stream = -1; run->roc = 0; run->seq = 0; run->ssrc = 0; }
// THE send rule: datagram i -> its run and its verdict (OK: the index is taken, cipher and MAC follow); a datagram that may not leave is
// voided here.  One lane per listed stream, and the list is strictly increasing (build's check stands behind build_count): no two lanes
// share a send record
SX_HD i32 sx_srtcp_protect_plan(const SxSrtcpProtectArgs& a, int i, SxSrtpRun* run) {
    const SxRtpDgram d = a.dgrams[i];
    sx_srtcp_run_clear(run);
    if (d.len == 0) return run->verdict = SX_SRTP_SKIPPED;
    const i32 s = a.streams[i];
    const bool other = a.keys && s >= 0 && s < a.n_streams && sx_srtp_key(a.keys, s, 0)->transform != SX_SRTP_CM;
    if (other && a.gcm) return run->verdict = SX_SRTCP_ELSEWHERE;
    const SxRtpDgram none = {0, 0};
    a.dgrams[i] = none;                                     // (written again behind the MAC)
    if (d.len < SX_SRTCP_HEAD || (d.len & 3) || d.offset < 0 || (i64)d.offset + (i64)d.len + SX_SRTCP_TRAILER > a.wire_bytes || s < 0 || s >= a.n_streams)
        return run->verdict = SX_SRTP_MALFORMED;
    if (!a.keys || !sx_srtp_key(a.keys, s, 0)->has || other) return run->verdict = SX_SRTP_NO_KEY;
    const u32 index = a.tx[s].next;
    if (index >= SX_SRTCP_INDEX_END) return run->verdict = SX_SRTCP_EXHAUSTED;
    a.tx[s].next = index + 1u;
    const u8* lo = a.wire + d.offset;
    run->off = d.offset; run->len = d.len; run->hdr = SX_SRTCP_HEAD; run->stream = s;
    run->roc = index >> 16; run->seq = index & 0xFFFFu; run->ssrc = sx_rtp_be32(lo + 4, lo, lo + d.len);
    return run->verdict = SX_SRTP_OK;
}
SX_HD void sx_srtcp_cipher(u8* wire, const SxSrtpKey* keys, int dir, const SxSrtpRun& r, const u32* te, int lane, int nlanes) {
    sx_srtp_cipher(wire + r.off, r.hdr, r.len, sx_srtp_key(keys, r.stream, dir), te, r.ssrc, r.roc, r.seq, lane, nlanes);
}
// the E || index word and the tag behind the packet, and the datagram's entry with both counted in
SX_HD void sx_srtcp_protect_mac(const SxSrtcpProtectArgs& a, int i, const SxSrtpRun& r) {
    const SxSrtpKey* key = sx_srtp_key(a.keys, r.stream, 0);
    const u32 word = 0x80000000u | (r.roc << 16) | r.seq;
    u32 tag[5];
    u8* p = a.wire + r.off;
    sx_srtp_mac(key->mid_i, key->mid_o, p, r.len, word, 4, tag);
#pragma unroll
    for (int b = 0; b < 4; b++) p[r.len + b] = (u8)(word >> (8 * (3 - b)));
#pragma unroll
    for (int b = 0; b < SX_SRTCP_TAG; b++) p[r.len + 4 + b] = (u8)sx_srtp_tag_byte(tag, b);
    SxRtpDgram d; d.offset = r.off; d.len = r.len + SX_SRTCP_TRAILER;
    a.dgrams[i] = d;
}

// ---- unprotect ---------------------------------------------------------------------------------------------------------------------------
struct SxSrtcpUnprotectArgs {
    const SxRtpDgram* dgrams; SxRtpDgram* out; u8* wire; const u32* table; const SxSrtpKey* keys; SxSrtcpRx* rx;      // keys, rx: NULL = no stream has a key
    i64 wire_bytes;                                          // (at most 2^31 - 1)
    int n_dgrams, n_streams;
    int gcm = 0;                                             // the GCM kernel follows this one (solo_srtp_gcm.h): see SX_SRTP_ELSEWHERE
};
// THE receive rule: datagram i -> its run and its verdict, the first rule that fails; authenticated here, by this lane.  d_dgrams_out[i]
// is written either way, and the stream's pending index is raised for an accepted datagram.  A run with E = 0 has hdr = len: no cipher
SX_HD i32 sx_srtcp_unprotect_one(const SxSrtcpUnprotectArgs& a, int i, SxSrtpRun* run) {
    const SxRtpDgram d = a.dgrams[i];
    const SxRtpDgram none = {0, 0};
    a.out[i] = none;
    sx_srtcp_run_clear(run);
    if (d.len < SX_SRTCP_HEAD + SX_SRTCP_TRAILER || d.offset < 0 || (i64)d.offset + (i64)d.len > a.wire_bytes) return run->verdict = SX_SRTP_MALFORMED;
    const u8* lo = a.wire + d.offset;
    const u8* hi = lo + d.len;
    const u32 ssrc = sx_rtp_be32(lo + 4, lo, hi);
    i32 stream = sx_rtp_find_ssrc(a.table, ssrc);
    if (stream < 0 || stream >= a.n_streams) return run->verdict = SX_SRTP_UNKNOWN_SSRC;
    if (!a.keys || !a.rx || !sx_srtp_key(a.keys, stream, 1)->has) return run->verdict = SX_SRTP_NO_KEY;
    const SxSrtpKey* key = sx_srtp_key(a.keys, stream, 1);
    if (key->transform != SX_SRTP_CM) {
        if (!a.gcm) return run->verdict = SX_SRTP_NO_KEY;   // (no kernel behind this one: no key this call can use)
        if (a.out == a.dgrams) a.out[i] = d;                // the kernel behind reads dgrams[i]: where out IS dgrams the entry goes back
        return run->verdict = SX_SRTCP_ELSEWHERE;
    }
    const i32 body = d.len - SX_SRTCP_TRAILER;               // what the tag covers, with the word behind it
    const u32 word = sx_rtp_be32(lo + body, lo, hi), index = word & 0x7FFFFFFFu;
    if ((i64)index <= a.rx[stream].index) return run->verdict = SX_SRTCP_REPLAYED;
    u32 tag[5];
    sx_srtp_mac(key->mid_i, key->mid_o, lo, body, word, 4, tag);
    u32 diff = 0;
#pragma unroll
    for (int b = 0; b < SX_SRTCP_TAG; b++) diff |= sx_srtp_tag_byte(tag, b) ^ (u32)lo[body + 4 + b];
    if (diff) return run->verdict = SX_SRTP_AUTH_FAILED;
    run->off = d.offset; run->len = body; run->hdr = (word >> 31) ? SX_SRTCP_HEAD : body; run->stream = stream;
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

#if defined(__HIPCC__)
__device__ __forceinline__ void sx_srtcp_count_flush(const i32* cnt, i32* count) {
    const int tid = (int)threadIdx.x;
    if (tid < 8 && cnt[tid]) atomicAdd(&count[tid], cnt[tid]);
}
// The count is zeroed by solo_rtp_clear_kernel ahead of either kernel, as in solo_srtp.h
__global__ void __launch_bounds__(SX_RTP_TILE) solo_srtcp_protect_kernel(const SxSrtcpProtectArgs a, i32* count) {
    __shared__ u32 te[256];
    __shared__ i32 cnt[16];                                 // (8 .. : SX_SRTCP_ELSEWHERE)
    __shared__ SxSrtpRun runs[SX_RTP_TILE];
    if (sx_srtcp_refused(a)) {
        if (blockIdx.x == 0 && threadIdx.x == 0) count[0] = -1;
        return;
    }
    const int tid = (int)threadIdx.x;
    const int i = (int)blockIdx.x * SX_RTP_TILE + tid;
    te[tid] = SX_AES_TE0_DEV[tid];
    if (tid < 16) cnt[tid] = 0;
    __syncthreads();
    SxSrtpRun run;
    sx_srtcp_run_clear(&run); run.verdict = -1;
    if (i < a.n) atomicAdd(&cnt[sx_srtcp_protect_plan(a, i, &run)], 1);
    runs[tid] = run;
    __syncthreads();
    const int lane = tid & (SX_RTP_ROW - 1);
    for (int t = tid / SX_RTP_ROW; t < SX_RTP_TILE; t += SX_RTP_TILE / SX_RTP_ROW) {
        const SxSrtpRun r = runs[t];
        if (r.verdict == SX_SRTP_OK) sx_srtcp_cipher(a.wire, a.keys, 0, r, te, lane, SX_RTP_ROW);
    }
    __syncthreads();                                        // (the ciphertext of this tile is written: the MAC reads it)
    if (run.verdict == SX_SRTP_OK) sx_srtcp_protect_mac(a, i, run);
    sx_srtcp_count_flush(cnt, count);
}
__global__ void __launch_bounds__(SX_RTP_TILE) solo_srtcp_unprotect_kernel(const SxSrtcpUnprotectArgs a, i32* count) {
    __shared__ u32 te[256];
    __shared__ i32 cnt[16];                                 // (8 .. : SX_SRTCP_ELSEWHERE)
    __shared__ SxSrtpRun runs[SX_RTP_TILE];
    const int tid = (int)threadIdx.x;
    const int i = (int)blockIdx.x * SX_RTP_TILE + tid;
    te[tid] = SX_AES_TE0_DEV[tid];
    if (tid < 16) cnt[tid] = 0;
    __syncthreads();
    SxSrtpRun run;
    sx_srtcp_run_clear(&run); run.verdict = -1;
    if (i < a.n_dgrams) atomicAdd(&cnt[sx_srtcp_unprotect_one(a, i, &run)], 1);
    runs[tid] = run;
    __syncthreads();
    const int lane = tid & (SX_RTP_ROW - 1);
    for (int t = tid / SX_RTP_ROW; t < SX_RTP_TILE; t += SX_RTP_TILE / SX_RTP_ROW) {
        const SxSrtpRun r = runs[t];
        if (r.verdict == SX_SRTP_OK) sx_srtcp_cipher(a.wire, a.keys, 1, r, te, lane, SX_RTP_ROW);
    }
    sx_srtcp_count_flush(cnt, count);
}
__global__ void __launch_bounds__(SX_RTP_TILE) solo_srtcp_rx_fold_kernel(SxSrtcpRx* rx, int n_streams) {
    const int s = (int)blockIdx.x * SX_RTP_TILE + (int)threadIdx.x;
    if (s < n_streams) sx_srtp_rx_fold(rx, s);
}
static inline hipError_t solo_srtcp_protect_launch(const SxSrtcpProtectArgs& a, SxSrtcpCount* count, hipStream_t s) {
    hipLaunchKernelGGL(solo_rtp_clear_kernel, dim3(1), dim3(64), 0, s, (i32*)count);
    hipLaunchKernelGGL(solo_srtcp_protect_kernel, dim3((a.n + SX_RTP_TILE - 1) / SX_RTP_TILE), dim3(SX_RTP_TILE), 0, s, a, (i32*)count);
    return hipGetLastError();
}
// the two halves of an unprotect call, as in solo_srtp.h
static inline hipError_t solo_srtcp_unprotect_launch_verdicts(const SxSrtcpUnprotectArgs& a, SxSrtcpCount* count, hipStream_t s) {
    hipLaunchKernelGGL(solo_rtp_clear_kernel, dim3(1), dim3(64), 0, s, (i32*)count);
    if (a.n_dgrams == 0) return hipGetLastError();
    hipLaunchKernelGGL(solo_srtcp_unprotect_kernel, dim3((a.n_dgrams + SX_RTP_TILE - 1) / SX_RTP_TILE), dim3(SX_RTP_TILE), 0, s, a, (i32*)count);
    return hipGetLastError();
}
static inline hipError_t solo_srtcp_unprotect_launch_fold(const SxSrtcpUnprotectArgs& a, hipStream_t s) {
    if (a.n_dgrams == 0 || !a.rx) return hipSuccess;
    hipLaunchKernelGGL(solo_srtcp_rx_fold_kernel, dim3((a.n_streams + SX_RTP_TILE - 1) / SX_RTP_TILE), dim3(SX_RTP_TILE), 0, s, a.rx, a.n_streams);
    return hipGetLastError();
}
static inline hipError_t solo_srtcp_unprotect_launch(const SxSrtcpUnprotectArgs& a, SxSrtcpCount* count, hipStream_t s) {
    const hipError_t e = solo_srtcp_unprotect_launch_verdicts(a, count, s);
    return e != hipSuccess ? e : solo_srtcp_unprotect_launch_fold(a, s);
}
#else
// Host forms (tests): tile by tile, phase by phase, lane by lane through the per-datagram functions above.
static inline void sx_srtcp_protect_host(const SxSrtcpProtectArgs& a, SxSrtcpCount* count) {
    i32 c[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (sx_srtcp_refused(a)) { c[0] = -1; memcpy(count, c, sizeof(*count)); return; }
    SxSrtpRun* runs = new SxSrtpRun[SX_RTP_TILE];
    for (int t0 = 0; t0 < a.n; t0 += SX_RTP_TILE) {
        const int m = sx_min(a.n - t0, SX_RTP_TILE);
        for (int t = 0; t < m; t++) c[sx_srtcp_protect_plan(a, t0 + t, &runs[t])]++;
        for (int t = 0; t < m; t++)
            for (int lane = 0; lane < SX_RTP_ROW && runs[t].verdict == SX_SRTP_OK; lane++) sx_srtcp_cipher(a.wire, a.keys, 0, runs[t], SX_AES_TE0, lane, SX_RTP_ROW);
        for (int t = 0; t < m; t++)
            if (runs[t].verdict == SX_SRTP_OK) sx_srtcp_protect_mac(a, t0 + t, runs[t]);
    }
    delete[] runs;
    memcpy(count, c, sizeof(*count));
}
static inline void sx_srtcp_unprotect_host(const SxSrtcpUnprotectArgs& a, SxSrtcpCount* count) {
    i32 c[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    SxSrtpRun* runs = new SxSrtpRun[SX_RTP_TILE];
    for (int t0 = 0; t0 < a.n_dgrams; t0 += SX_RTP_TILE) {
        const int m = sx_min(a.n_dgrams - t0, SX_RTP_TILE);
        for (int t = 0; t < m; t++) c[sx_srtcp_unprotect_one(a, t0 + t, &runs[t])]++;
        for (int t = 0; t < m; t++)
            for (int lane = 0; lane < SX_RTP_ROW && runs[t].verdict == SX_SRTP_OK; lane++) sx_srtcp_cipher(a.wire, a.keys, 1, runs[t], SX_AES_TE0, lane, SX_RTP_ROW);
    }
    if (a.rx)
        for (int s = 0; s < a.n_streams; s++) sx_srtp_rx_fold(a.rx, s);
    delete[] runs;
    memcpy(count, c, sizeof(*count));
}
#endif

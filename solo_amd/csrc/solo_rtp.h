// solo_rtp.h -- RTP at both ends of the bridge (solo_rtp_pack, solo_rtp_parse; include/solo_mi355x.h): the records and the pool of
// solo_send_pack / solo_send_fanout -> datagrams with an RTP header (RFC 3550 section 5.1) in front, ready for the socket, and received
// datagrams -> the arrivals solo_recv_insert takes, in place.  The RFC 6464 audio level that solo_vad / solo_agc compute travels in a
// one-byte header extension (RFC 8285 section 4.2) and is read back without decoding.
//
// A session (solo_rtp_t, solo_api.hip) holds per stream FOUR words on the device -- {SSRC, timestamp offset, sequence offset | PT of
// MD1 << 16 | PT of MD2 || HB << 24, bound} -- and one table: {bound streams, level id, 0, 0}, then the (ssrc, stream) pairs of the
// bound streams sorted by SSRC.  The device code reads both and writes neither: with the configuration held fixed, pack and parse are
// pure functions of their inputs.
//
// Pack: datagram k belongs to record k.  Offsets of the pool may repeat (fanout stores a source datagram once), so the wire offsets are
// a prefix sum of roundup4(H + len + T) over the valid records, H = 12 or 20, T the session's trailer (solo_rtp_set_trailer: room for the
// SRTP tag of solo_srtp.h, written as zero; 0 unless asked for): three short launches, as in solo_send.h, none of which waits
// for another workgroup:
//     1. totals   one workgroup per tile of SX_RTP_TILE records (a lane per record): {valid, refused} and padded bytes of the tile
//     2. scan     ONE wavefront walks the tile totals 64 at a time (wv_scan_incl) -> every tile's first wire offset, the call's counts
//     3. scatter  the tile again: the same plan per record, a scan inside the tile (wg_scan_incl), the d_dgrams entry by the record's
//                 lane, then the bytes by a 16-lane row per datagram: header dwords, payload (sx_send_copy, solo_send.h: the
//                 destination is dword-aligned by construction, the source is not), zero pad bytes
// Every datagram starts at a multiple of 4, so the header goes out as whole dwords and the copy has no head; the 0 .. 3 bytes behind a
// datagram are written as zero.  The record count is min(send_count->records, max_records), read on the device.
//
// Parse: one kernel, a lane per datagram, no compaction; the header is composed from aligned dword loads clipped to the datagram
// (sx_send_ld_clipped), the extension elements are walked byte by byte inside the block.
//
// Everything below compiles for the host as well (tests/test_rtp_model.py builds the host forms and compares them with an independent
// model).
#pragma once
#include <string.h>
#include <algorithm>
#include "solo_send.h"
#include "solo_recv.h"

#define SX_RTP_TILE 256         // records per tile = lanes per workgroup of pack's passes 1 and 3, and of the parse kernel
#define SX_RTP_ROW 16           // lanes that write one datagram
#define SX_RTP_CFG_WORDS 4      // a stream's configuration record
#define SX_RTP_TABLE_HEAD 4     // words in front of the (ssrc, stream) pairs

// what became of a received datagram: the FIRST rule that fails, in this order (== the fields of solo_rtp_parse_count_t behind `with_level`)
#define SX_RTP_ACCEPTED 0
#define SX_RTP_MALFORMED 1
#define SX_RTP_VERSION 2
#define SX_RTP_UNKNOWN_SSRC 3
#define SX_RTP_UNKNOWN_PT 4
#define SX_RTP_TIMESTAMP 5

typedef solo_dgram_t SxRtpDgram;
static_assert(sizeof(SxRtpDgram) == 8, "solo_dgram_t layout");
typedef solo_rtp_pack_count_t SxRtpPackCount;
static_assert(sizeof(SxRtpPackCount) == 32, "solo_rtp_pack_count_t layout");
typedef solo_rtp_parse_count_t SxRtpParseCount;
static_assert(sizeof(SxRtpParseCount) == 32, "solo_rtp_parse_count_t layout");

struct SxRtpStream { u32 ssrc, ts_offset, seq_pt, bound; };  // a stream's record; seq_pt: sequence offset | pt_md1 << 16 | pt_md2 << 24
static_assert(sizeof(SxRtpStream) == 4 * SX_RTP_CFG_WORDS, "a stream's RTP record");

// ---- the control plane: the host mirror of a session, what a bind or unbind call makes of it (solo_api.hip and the tests both ask here) ----
struct SxRtpMirror {
    std::vector<SxRtpStream> cfg;                            // [n_streams]
    i32 level_id;
};
// the device table of a configuration: {bound streams, level id, 0, 0}, then the (ssrc, stream) pairs sorted by SSRC.  false: an SSRC twice
static inline bool sx_rtp_table(const std::vector<SxRtpStream>& cfg, i32 level_id, std::vector<u32>& table) {
    std::vector<unsigned long long> keys;
    for (size_t s = 0; s < cfg.size(); s++)
        if (cfg[s].bound) keys.push_back(((unsigned long long)cfg[s].ssrc << 32) | (unsigned long long)s);
    std::sort(keys.begin(), keys.end());
    table.assign(SX_RTP_TABLE_HEAD + 2 * cfg.size(), 0u);
    table[0] = (u32)keys.size(); table[1] = (u32)level_id;
    for (size_t i = 0; i < keys.size(); i++) {
        if (i > 0 && (keys[i] >> 32) == (keys[i - 1] >> 32)) return false;
        table[SX_RTP_TABLE_HEAD + 2 * i] = (u32)(keys[i] >> 32); table[SX_RTP_TABLE_HEAD + 2 * i + 1] = (u32)keys[i];
    }
    return true;
}
// A bind call: everything is validated before anything changes.  -> false: refused; true: `next` is the mirror after the call, recs holds
// one record per listed stream (solo_rtp_bind_kernel) and table the new device table.  The mirror itself is not touched: the caller
// commits `next` once the device holds the records and the table, so that a call that fails on the device leaves the mirror where the
// device was and the duplicate-SSRC rule keeps judging what the device has
static inline bool sx_rtp_bind_plan(const SxRtpMirror& m, const int32_t* streams, int32_t n, const uint32_t* ssrc, const uint32_t* ts_offset,
                                    const uint16_t* seq_offset, const uint8_t* pt_md1, const uint8_t* pt_md2, int32_t level_id, SxRtpMirror& next,
                                    std::vector<SxStreamCtl>& recs, std::vector<u32>& table) {
    if (!ssrc || !ts_offset || !seq_offset || !pt_md1 || !pt_md2 || level_id < 0 || level_id > 14 || !sx_list_ok(streams, n, (int32_t)m.cfg.size())) return false;
    next.cfg = m.cfg; next.level_id = level_id;
    recs.resize((size_t)n);
    for (int32_t i = 0; i < n; i++) {
        if (pt_md1[i] > 127 || pt_md2[i] > 127) return false;
        SxRtpStream c; c.ssrc = ssrc[i]; c.ts_offset = ts_offset[i]; c.seq_pt = (u32)seq_offset[i] | ((u32)pt_md1[i] << 16) | ((u32)pt_md2[i] << 24); c.bound = 1;
        next.cfg[(size_t)streams[i]] = c;
        recs[(size_t)i] = SxStreamCtl{streams[i], (int32_t)c.ssrc, (int32_t)c.ts_offset, (int32_t)c.seq_pt};
    }
    return sx_rtp_table(next.cfg, level_id, table);
}
// An unbind call, likewise (a listed stream that is not bound stays so)
static inline bool sx_rtp_unbind_plan(const SxRtpMirror& m, const int32_t* streams, int32_t n, SxRtpMirror& next, std::vector<u32>& table) {
    if (!sx_list_ok(streams, n, (int32_t)m.cfg.size())) return false;
    next = m;
    for (int32_t i = 0; i < n; i++) { const SxRtpStream z = {0, 0, 0, 0}; next.cfg[(size_t)streams[i]] = z; }
    return sx_rtp_table(next.cfg, next.level_id, table);
}

SX_HD u32 sx_rtp_bswap(u32 v) { return (v >> 24) | ((v >> 8) & 0xFF00u) | ((v << 8) & 0xFF0000u) | (v << 24); }
SX_HD i32 sx_rtp_roundup4(i32 n) { return (n + 3) & ~3; }

// ---- pack ------------------------------------------------------------------------------------------------------------------------
struct SxRtpPackArgs {
    const SxSendRecord* records; const SxSendCount* send_count; const u8* payload; const u8* level; const SxRtpStream* cfg; const u32* table;
    i64 payload_bytes;
    int max_records, n_streams, level_depth, packet_samples;
    int trailer = 0;                                        // bytes kept free behind every datagram (solo_rtp_set_trailer: the SRTP tag's room), written as zero
};
struct SxRtpRun { i32 src, dst, len; u32 w0, ts, ssrc, ext, pad; };   // one datagram of pass 3: payload[src ..) -> wire[dst + H ..), the header's words
static_assert(sizeof(SxRtpRun) == 32, "a run in LDS");

// records of the call, read on the device: < 0 = the list behind the records was refused
SX_HD i32 sx_rtp_n_records(const SxRtpPackArgs& a) { return sx_min(a.send_count->records, a.max_records); }
SX_HD int sx_rtp_header_bytes(const SxRtpPackArgs& a) { return a.level ? 20 : 12; }
// what a datagram of wlen bytes takes of the wire: itself, the trailer and the pad bytes up to a multiple of 4 (0 for a refused record)
SX_HD i32 sx_rtp_padded(const SxRtpPackArgs& a, i32 wlen) { return wlen > 0 ? sx_rtp_roundup4(wlen + a.trailer) : 0; }

// THE record rule: record k -> bytes of its datagram, header included (0: refused; its payload is never read), and where asked for the
// header's words as they are stored (little-endian dwords of the big-endian fields)
SX_HD i32 sx_rtp_pack_plan(const SxRtpPackArgs& a, int k, SxRtpRun* run) {
    const SxSendRecord r = a.records[k];
    if (r.stream < 0 || r.stream >= a.n_streams || r.desc < 0 || r.desc > 1 || r.seq < 0 || r.len <= 0 || r.len > 32767 || r.offset < 0 ||
        (i64)r.offset + (i64)r.len > a.payload_bytes)
        return 0;
    const SxRtpStream c = a.cfg[r.stream];
    if (!c.bound) return 0;
    if (run) {
        const u32 pt = (c.seq_pt >> (16 + 8 * r.desc)) & 127u;
        const u32 seq = (c.seq_pt + 2u * (u32)r.seq + (u32)r.desc) & 0xFFFFu;
        run->src = r.offset; run->len = r.len; run->dst = 0;
        run->pad = (u32)(sx_rtp_padded(a, sx_rtp_header_bytes(a) + r.len) - sx_rtp_header_bytes(a) - r.len);    // trailer and pad bytes
        run->w0 = (a.level ? 0x90u : 0x80u) | (pt << 8) | ((seq >> 8) << 16) | ((seq & 255u) << 24);
        run->ts = sx_rtp_bswap(c.ts_offset + (u32)r.seq * (u32)a.packet_samples);
        run->ssrc = sx_rtp_bswap(c.ssrc);
        run->ext = a.level ? ((a.table[1] & 15u) << 4) | ((u32)a.level[sx_recv_entry(r.stream, r.seq, a.level_depth)] << 8) : 0;
    }
    return sx_rtp_header_bytes(a) + r.len;
}
// what a record adds to the tile totals: valid | refused << 10 (each at most SX_RTP_TILE per tile)
SX_HD i32 sx_rtp_pack_counts(i32 wlen) { return wlen > 0 ? 1 : (1 << 10); }

// a datagram of `wlen` bytes (`padded` with its trailer and pad bytes) at wire offset `off` is written iff all of that ends inside cap
// (<= 2^31 - 1).  The offsets grow along the order, so what is written is a prefix.  d_dgrams[k] is written either way: {0, 0} for a
// datagram that is not; its len is wlen, the RTP packet without the trailer
SX_HD bool sx_rtp_pack_emit(SxRtpDgram* dgrams, int k, i32 wlen, i32 padded, i64 off, i64 cap) {
    const bool w = wlen > 0 && off + (i64)padded <= cap;
    SxRtpDgram d; d.offset = w ? (i32)off : 0; d.len = w ? wlen : 0;
    dgrams[k] = d;
    return w;
}
// the bytes of one datagram by `nlanes` lanes, this one being `lane`: header dwords, payload, zero trailer and pad (dst is dword-aligned)
SX_HD void sx_rtp_write(u8* dst, const u8* payload, const SxRtpRun& r, int H, int lane, int nlanes) {
    u32* d32 = (u32*)dst;
    if (lane == 0) d32[0] = r.w0;
    if (lane == 1) d32[1] = r.ts;
    if (lane == 2) d32[2] = r.ssrc;
    if (H == 20) {
        if (lane == 3) d32[3] = 0x0100DEBEu;                // 0xBE 0xDE, length 1 (in 32-bit words)
        if (lane == 4) d32[4] = r.ext;                      // id << 4 | (len - 1 = 0), the level byte, two pad bytes
    }
    sx_send_copy(dst + H, payload + r.src, r.len, lane, nlanes);
    const int end = H + r.len;
    for (int i = lane; i < (int)r.pad; i += nlanes) dst[end + i] = 0;
}

struct SxRtpBase { i64 bytes; };                            // where a tile's output starts

#if defined(__HIPCC__)
// pass 1: totals[tile] = {counts (packed as sx_rtp_pack_counts), padded bytes}
__global__ void __launch_bounds__(SX_RTP_TILE) solo_rtp_totals_kernel(const SxRtpPackArgs a, i32* __restrict__ totals) {
    __shared__ i32 red[4];
    const i32 n = sx_rtp_n_records(a);
    if (n < 0) return;
    const int k = (int)blockIdx.x * SX_RTP_TILE + (int)threadIdx.x;
    i32 cnt = 0, bytes = 0;
    if (k < n) {
        const i32 wlen = sx_rtp_pack_plan(a, k, NULL);
        cnt = sx_rtp_pack_counts(wlen);
        bytes = sx_rtp_padded(a, wlen);
    }
    cnt = wg_sum(cnt, red);
    bytes = wg_sum(bytes, red);
    if (threadIdx.x == 0) { totals[blockIdx.x * 2 + 0] = cnt; totals[blockIdx.x * 2 + 1] = bytes; }
}
// pass 2: one wavefront; a tile holds at most 256 x 32804 bytes, so 64 of them scan in 32 bits and the running base is carried in 64
__global__ void __launch_bounds__(64) solo_rtp_scan_kernel(const SxRtpPackArgs a, const i32* __restrict__ totals, SxRtpBase* __restrict__ bases, int n_tiles,
                                                           SxRtpPackCount* count) {
    if (sx_rtp_n_records(a) < 0) {
        if (threadIdx.x == 0) count->dgrams = -1;
        return;
    }
    i64 byte_base = 0;
    i32 valid = 0, refused = 0;
    for (int t0 = 0; t0 < n_tiles; t0 += 64) {
        const int t = t0 + (int)threadIdx.x;
        const i32 cnt = t < n_tiles ? totals[t * 2 + 0] : 0, bytes = t < n_tiles ? totals[t * 2 + 1] : 0;
        const i32 ibytes = wv_scan_incl(bytes);
        if (t < n_tiles) bases[t].bytes = byte_base + (i64)(ibytes - bytes);
        byte_base += (i64)__builtin_amdgcn_readlane(ibytes, 63);
        valid += wv_sum(cnt & 1023);
        refused += wv_sum((cnt >> 10) & 1023);
    }
    if (threadIdx.x == 0) {         // (datagrams / bytes WRITTEN: pass 3 adds what each tile wrote)
        SxRtpPackCount c; c.dgrams = 0; c.dgrams_needed = valid; c.bytes = 0; c.bytes_needed = byte_base; c.refused = refused; c.reserved = 0;
        *count = c;
    }
}
// pass 3: the d_dgrams entry by the record's lane, then the bytes by a 16-lane row per datagram
__global__ void __launch_bounds__(SX_RTP_TILE) solo_rtp_scatter_kernel(const SxRtpPackArgs a, const SxRtpBase* __restrict__ bases, SxRtpDgram* __restrict__ dgrams,
                                                                       u8* __restrict__ wire, long long cap, SxRtpPackCount* count) {
    __shared__ i32 red[4], part[1][4];
    __shared__ SxRtpRun runs[SX_RTP_TILE];
    const i32 n = sx_rtp_n_records(a);
    if (n < 0) return;
    const int tid = (int)threadIdx.x;
    const int k = (int)blockIdx.x * SX_RTP_TILE + tid;
    SxRtpRun run;
    run.src = 0; run.dst = 0; run.len = 0; run.w0 = 0; run.ts = 0; run.ssrc = 0; run.ext = 0; run.pad = 0;
    i32 wlen = 0;
    if (k < n) wlen = sx_rtp_pack_plan(a, k, &run);
    const i32 bytes = sx_rtp_padded(a, wlen);
    const i32 ibytes = wg_scan_incl(bytes, part);
    bool written = false;
    if (k < n) {
        const i64 off = bases[blockIdx.x].bytes + (i64)(ibytes - bytes);
        written = sx_rtp_pack_emit(dgrams, k, wlen, bytes, off, cap);
        run.dst = (i32)off;
    }
    if (!written) run.len = 0;
    runs[tid] = run;
    const i32 tile_written = wg_sum((i32)written, red), tile_bytes = wg_sum(written ? bytes : 0, red);     // (its barriers publish runs[])
    if (tid == 0 && tile_written) {
        atomicAdd(&count->dgrams, tile_written);
        atomicAdd((unsigned long long*)&count->bytes, (unsigned long long)tile_bytes);
    }
    const int H = sx_rtp_header_bytes(a), lane = tid & (SX_RTP_ROW - 1);
    for (int t = tid / SX_RTP_ROW; t < SX_RTP_TILE; t += SX_RTP_TILE / SX_RTP_ROW) {
        const SxRtpRun r = runs[t];
        if (r.len > 0) sx_rtp_write(wire + r.dst, a.payload, r, H, lane, SX_RTP_ROW);
    }
}

// bytes of device scratch a call over max_records records needs: the tile bases, then the tile totals
static inline size_t solo_rtp_scratch_bytes(int max_records) {
    const size_t n_tiles = ((size_t)max_records + SX_RTP_TILE - 1) / SX_RTP_TILE;
    return n_tiles * (sizeof(SxRtpBase) + 2 * sizeof(i32));
}
static inline hipError_t solo_rtp_pack_launch(const SxRtpPackArgs& a, void* scratch, SxRtpDgram* dgrams, u8* wire, long long cap, SxRtpPackCount* count,
                                              hipStream_t s) {
    const int n_tiles = (a.max_records + SX_RTP_TILE - 1) / SX_RTP_TILE;
    SxRtpBase* bases = (SxRtpBase*)scratch;
    i32* totals = (i32*)(bases + n_tiles);
    if (cap > 0x7FFFFFFFLL) cap = 0x7FFFFFFFLL;
    hipLaunchKernelGGL(solo_rtp_totals_kernel, dim3(n_tiles), dim3(SX_RTP_TILE), 0, s, a, totals);
    hipLaunchKernelGGL(solo_rtp_scan_kernel, dim3(1), dim3(64), 0, s, a, totals, bases, n_tiles, count);
    hipLaunchKernelGGL(solo_rtp_scatter_kernel, dim3(n_tiles), dim3(SX_RTP_TILE), 0, s, a, bases, dgrams, wire, cap, count);
    return hipGetLastError();
}
#else
// Host form of the three passes (tests): tile by tile, lane by lane, through the per-record functions above.
static inline void sx_rtp_pack_host(const SxRtpPackArgs& a, SxRtpDgram* dgrams, u8* wire, long long cap, SxRtpPackCount* count) {
    const i32 n = sx_rtp_n_records(a);
    if (n < 0) { count->dgrams = -1; return; }
    const int n_tiles = (a.max_records + SX_RTP_TILE - 1) / SX_RTP_TILE, H = sx_rtp_header_bytes(a);
    if (cap > 0x7FFFFFFFLL) cap = 0x7FFFFFFFLL;
    i32* totals = new i32[(size_t)n_tiles * 2];
    SxRtpBase* bases = new SxRtpBase[(size_t)n_tiles];
    for (int t = 0; t < n_tiles; t++) {                     // pass 1
        i32 cnt = 0, bytes = 0;
        for (int k = t * SX_RTP_TILE; k < n && k < (t + 1) * SX_RTP_TILE; k++) {
            const i32 wlen = sx_rtp_pack_plan(a, k, NULL);
            cnt += sx_rtp_pack_counts(wlen);
            bytes += sx_rtp_padded(a, wlen);
        }
        totals[t * 2 + 0] = cnt; totals[t * 2 + 1] = bytes;
    }
    SxRtpPackCount c; c.dgrams = 0; c.dgrams_needed = 0; c.bytes = 0; c.bytes_needed = 0; c.refused = 0; c.reserved = 0;
    for (int t = 0; t < n_tiles; t++) {                     // pass 2
        bases[t].bytes = c.bytes_needed;
        c.dgrams_needed += totals[t * 2] & 1023; c.refused += (totals[t * 2] >> 10) & 1023; c.bytes_needed += totals[t * 2 + 1];
    }
    for (int t = 0; t < n_tiles; t++) {                     // pass 3
        i64 off = bases[t].bytes;
        for (int k = t * SX_RTP_TILE; k < n && k < (t + 1) * SX_RTP_TILE; k++) {
            SxRtpRun run;
            const i32 wlen = sx_rtp_pack_plan(a, k, &run);
            if (sx_rtp_pack_emit(dgrams, k, wlen, sx_rtp_padded(a, wlen), off, cap)) {
                for (int lane = 0; lane < SX_RTP_ROW; lane++) sx_rtp_write(wire + off, a.payload, run, H, lane, SX_RTP_ROW);
                c.dgrams++; c.bytes += sx_rtp_padded(a, wlen);
            }
            off += sx_rtp_padded(a, wlen);
        }
    }
    *count = c;
    delete[] totals;
    delete[] bases;
}
#endif

// ---- parse -----------------------------------------------------------------------------------------------------------------------
struct SxRtpParseArgs {
    const SxRtpDgram* dgrams; const u8* wire; const SxRtpStream* cfg; const u32* table; const i32* play;
    i64 wire_bytes;                                          // (at most 2^31 - 1: an offset that is written fits its int32 field)
    int n_dgrams, n_streams, packet_samples;
};
struct SxRtpParsed { SxSendRecord arrival; i32 verdict; u32 level, rtp_seq; };

// the big-endian 32-bit word at p (any alignment), out of the two aligned dwords around it; only bytes inside [lo, hi) are read
SX_HD u32 sx_rtp_be32(const u8* p, const u8* lo, const u8* hi) {
    const u32 sh = (u32)((uintptr_t)p & 3);
    const u8* pa = p - (int)sh;
    u32 v = sx_send_ld_clipped(pa, lo, hi);
    if (sh) v = (v >> (8 * sh)) | (sx_send_ld_clipped(pa + 4, lo, hi) << (32 - 8 * sh));
    return sx_rtp_bswap(v);
}
// the stream bound to `ssrc`, or -1: binary search of the sorted pairs behind the table's head
SX_HD i32 sx_rtp_find_ssrc(const u32* table, u32 ssrc) {
    const u32* pairs = table + SX_RTP_TABLE_HEAD;
    i32 lo = 0, hi = (i32)table[0];
    while (lo < hi) {
        const i32 mid = (lo + hi) >> 1;
        if (pairs[2 * mid] < ssrc) lo = mid + 1;
        else hi = mid;
    }
    return (lo < (i32)table[0] && pairs[2 * lo] == ssrc) ? (i32)pairs[2 * lo + 1] : -1;
}
// the RFC 6464 byte of a one-byte-header extension block x[0 .. n) (RFC 8285 section 4.2): the first element with id `level_id` and one
// data byte; 255 = none.  Id 0 is a pad byte, id 15 ends the walk, and so does an element that reaches over the block's end.
SX_HD u32 sx_rtp_find_level(const u8* x, int n, u32 level_id) {
    int at = 0;
    while (at < n) {
        const u32 e = x[at];
        const u32 id = e >> 4;
        if (id == 0) { at++; continue; }
        if (id == 15) break;
        const int len = (int)(e & 15u) + 1;
        if (at + 1 + len > n) break;
        if (id == level_id && len == 1) return x[at + 1];
        at += 1 + len;
    }
    return 255u;
}
SX_HD SxRtpParsed sx_rtp_rejected(i32 verdict) {
    SxRtpParsed o;
    o.arrival.stream = -1; o.arrival.seq = 0; o.arrival.desc = 0; o.arrival.offset = 0; o.arrival.len = 0;
    o.verdict = verdict; o.level = 255u; o.rtp_seq = 0;
    return o;
}
// THE header walk, shared by parse and by both SRTP calls (solo_srtp.h): the datagram [lo, lo + len), len >= 12 -> bytes in front of the
// payload (12 + 4 CC, and with X set the extension block: 4 + 4 x its length), or -1 where that reaches past len.  w0: the first header
// word; ext_at / ext_len / profile: the extension block's body (0 without X)
struct SxRtpHead { u32 w0, profile; i32 ext_at, ext_len; };
SX_HD i32 sx_rtp_header_walk(const u8* lo, i32 len, SxRtpHead* h) {
    const u8* hi = lo + len;
    h->w0 = sx_rtp_be32(lo, lo, hi); h->profile = 0; h->ext_at = 0; h->ext_len = 0;
    i32 hdr = 12 + 4 * (i32)((h->w0 >> 24) & 15u);
    if (hdr > len) return -1;
    if ((h->w0 >> 28) & 1u) {
        if (hdr + 4 > len) return -1;
        const u32 xw = sx_rtp_be32(lo + hdr, lo, hi);
        h->profile = xw >> 16;
        h->ext_at = hdr + 4; h->ext_len = 4 * (i32)(xw & 0xFFFFu);
        hdr = h->ext_at + h->ext_len;
        if (hdr > len) return -1;
    }
    return hdr;
}
// THE datagram rule: datagram i -> its arrival, its verdict (the first rule that fails), its level byte and its raw sequence number
SX_HD SxRtpParsed sx_rtp_parse_one(const SxRtpParseArgs& a, int i) {
    const SxRtpDgram d = a.dgrams[i];
    if (d.len < 12 || d.offset < 0 || (i64)d.offset + (i64)d.len > a.wire_bytes) return sx_rtp_rejected(SX_RTP_MALFORMED);
    const u8* lo = a.wire + d.offset;
    const u8* hi = lo + d.len;
    SxRtpHead hd;
    const i32 hdr = sx_rtp_header_walk(lo, d.len, &hd);
    if (hdr < 0) return sx_rtp_rejected(SX_RTP_MALFORMED);
    const u32 w0 = hd.w0, profile = hd.profile;
    const i32 ext_at = hd.ext_at, ext_len = hd.ext_len;
    const bool has_x = ((w0 >> 28) & 1u) != 0, has_p = ((w0 >> 29) & 1u) != 0;
    i32 pad = 0;
    if (has_p) {
        pad = (i32)hi[-1];
        if (pad == 0 || pad > d.len - hdr) return sx_rtp_rejected(SX_RTP_MALFORMED);
    }
    const i32 len = d.len - hdr - pad;
    if (len <= 0 || len > 32767) return sx_rtp_rejected(SX_RTP_MALFORMED);
    if ((w0 >> 30) != 2u) return sx_rtp_rejected(SX_RTP_VERSION);
    const i32 stream = sx_rtp_find_ssrc(a.table, sx_rtp_be32(lo + 8, lo, hi));
    if (stream < 0 || stream >= a.n_streams) return sx_rtp_rejected(SX_RTP_UNKNOWN_SSRC);
    const SxRtpStream c = a.cfg[stream];
    const u32 pt = (w0 >> 16) & 127u, pt0 = (c.seq_pt >> 16) & 127u, pt1 = (c.seq_pt >> 24) & 127u;
    if (pt != pt0 && pt != pt1) return sx_rtp_rejected(SX_RTP_UNKNOWN_PT);
    // the packet number, unwrapped against the stream's play-out position
    const u32 L = (u32)a.packet_samples;
    const i32 p = a.play[stream];
    const i32 delta = (i32)(sx_rtp_be32(lo + 4, lo, hi) - c.ts_offset - (u32)p * L);
    if (delta % (i32)L != 0) return sx_rtp_rejected(SX_RTP_TIMESTAMP);
    const i64 seq = (i64)p + (i64)(delta / (i32)L);
    if (seq < 0 || seq > 0x7FFFFFFFLL) return sx_rtp_rejected(SX_RTP_TIMESTAMP);
    SxRtpParsed o;
    o.arrival.stream = stream; o.arrival.seq = (i32)seq; o.arrival.desc = pt0 == pt1 ? -1 : (pt == pt0 ? 0 : 1);
    o.arrival.offset = d.offset + hdr; o.arrival.len = len;
    o.verdict = SX_RTP_ACCEPTED; o.rtp_seq = w0 & 0xFFFFu;
    const u32 level_id = a.table[1];
    o.level = (has_x && profile == 0xBEDEu && level_id > 0) ? sx_rtp_find_level(lo + ext_at, ext_len, level_id) : 255u;
    return o;
}
// datagram i's outputs (level_out / rtp_seq_out: NULL = not wanted) -> the counter it adds to: 0 .. 5 = its verdict; bit 3: it carries a level
SX_HD int sx_rtp_parse_store(const SxRtpParseArgs& a, int i, SxSendRecord* arrivals, u8* level_out, uint16_t* rtp_seq_out) {
    const SxRtpParsed o = sx_rtp_parse_one(a, i);
    arrivals[i] = o.arrival;
    if (level_out) level_out[i] = (u8)o.level;
    if (rtp_seq_out) rtp_seq_out[i] = (uint16_t)o.rtp_seq;
    return o.verdict | ((o.verdict == SX_RTP_ACCEPTED && o.level != 255u) ? 8 : 0);
}
// verdict -> its word of SxRtpParseCount
SX_HD int sx_rtp_count_word(int verdict) { return verdict == SX_RTP_ACCEPTED ? 0 : verdict + 1; }

#if defined(__HIPCC__)
// The count of a parse call is zeroed by this kernel, ahead of the parse kernel.  NOT a hipMemsetAsync: with a memset node in front of the
// kernel, the count of a captured graph's replay differed from that of the same calls made eagerly (tests/test_gpu_rtp.py,
// test_capture_rtp_parse_and_recv_insert); with this kernel they are equal.  Why the memset node did that was not found, so do not put
// it back without that test
__global__ void __launch_bounds__(64) solo_rtp_clear_kernel(i32* count) {
    if (threadIdx.x < 8) count[threadIdx.x] = 0;
}
// One lane per datagram.  What bounds a lane: at most four header words (w0, the extension's first word, timestamp, SSRC), each out of
// two clipped dword loads; the pad count byte; a binary search of the bound table, log2(bound streams) + 1 dependent steps (13 at 4096);
// one load of the stream's record and one of its play-out position; and the walk over the extension block, one byte load per element
// or pad byte and at most min(len, 4 x 65535) steps.
__global__ void __launch_bounds__(SX_RTP_TILE) solo_rtp_parse_kernel(const SxRtpParseArgs a, SxSendRecord* __restrict__ arrivals, u8* __restrict__ level_out,
                                                                     uint16_t* __restrict__ rtp_seq_out, i32* count) {
    __shared__ i32 cnt[8];
    const int tid = (int)threadIdx.x;
    if (tid < 8) cnt[tid] = 0;
    __syncthreads();
    const int i = (int)blockIdx.x * SX_RTP_TILE + tid;
    if (i < a.n_dgrams) {
        const int v = sx_rtp_parse_store(a, i, arrivals, level_out, rtp_seq_out);
        atomicAdd(&cnt[sx_rtp_count_word(v & 7)], 1);
        if (v & 8) atomicAdd(&cnt[1], 1);
    }
    __syncthreads();
    if (tid < 7 && cnt[tid]) atomicAdd(&count[tid], cnt[tid]);
}
// a bind: the listed streams' records, by value (solo_stream_ctl.h: a = SSRC, b = timestamp offset, c = seq_pt); one workgroup per record
__global__ void __launch_bounds__(64) solo_rtp_bind_kernel(u32* cfg, const SxStreamCtlList l) {
    const SxStreamCtl r = l.r[blockIdx.x];
    if (threadIdx.x < SX_RTP_CFG_WORDS) {
        const u32 w[SX_RTP_CFG_WORDS] = {(u32)r.a, (u32)r.b, (u32)r.c, 1u};
        cfg[(size_t)r.stream * SX_RTP_CFG_WORDS + threadIdx.x] = w[threadIdx.x];
    }
}
static inline hipError_t solo_rtp_parse_launch(const SxRtpParseArgs& a, SxSendRecord* arrivals, u8* level_out, uint16_t* rtp_seq_out, SxRtpParseCount* count,
                                               hipStream_t s) {
    hipLaunchKernelGGL(solo_rtp_clear_kernel, dim3(1), dim3(64), 0, s, (i32*)count);
    if (a.n_dgrams == 0) return hipGetLastError();
    hipLaunchKernelGGL(solo_rtp_parse_kernel, dim3((a.n_dgrams + SX_RTP_TILE - 1) / SX_RTP_TILE), dim3(SX_RTP_TILE), 0, s, a, arrivals, level_out, rtp_seq_out,
                       (i32*)count);
    return hipGetLastError();
}
#else
static inline void sx_rtp_parse_host(const SxRtpParseArgs& a, SxSendRecord* arrivals, u8* level_out, uint16_t* rtp_seq_out, SxRtpParseCount* count) {
    i32 c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < a.n_dgrams; i++) {
        const int v = sx_rtp_parse_store(a, i, arrivals, level_out, rtp_seq_out);
        c[sx_rtp_count_word(v & 7)]++;
        if (v & 8) c[1]++;
    }
    memcpy(count, c, sizeof(*count));
}
#endif

// solo_fanout.h -- the sender back end for shared sources: ONE table of encoded packets, MANY destinations (solo_send_fanout,
// include/solo_mi355x.h).  Destination i sends the packets of source row d_source[i] under its own stream number, sequence numbers and
// mask; every source datagram is stored in the pool ONCE, however many destinations name it, and the records of those destinations carry
// the same offset.  This is the send step behind solo_mix_shared (the speakers' rows and the rooms' rows are the sources, every
// participant is a destination) and, on its own, a forwarding server's copy of one sender to many receivers.
//
// The length rules are those of solo_send_pack, through its one function (sx_send_plan, solo_send.h):
//     pool      per packet p (outer), then source row s, then description 0 before 1: the valid datagrams -- both descriptions, whatever
//               the masks say -- of every row that at least one destination names.  Rows nobody names are never read.
//     records   per packet p (outer), then destination i, then description 0 before 1: the rules applied to the source's length record
//               with the DESTINATION's mask and sequence number
//
// Six short launches, none of which waits for another workgroup:
//     1. clear    the `named` flags and the call's verdict word
//     2. mark     one lane per destination: a d_source outside [-1, n_src) sets the verdict (every later kernel then leaves before it
//                 touches anything); named[d_source[i]] = 1
//     3. totals   one workgroup per tile of SX_SEND_TILE packets, the source tiles first, then the destination tiles: pool bytes of a source
//                 tile, {records, empty, refused} of a destination tile
//     4. scan     ONE wavefront walks both runs of tile totals 64 at a time (solo_send_pack's kernel, solo_send_scan_kernel) -> every
//                 tile's base, the call's counts
//     5. pool     the source tiles again: a scan inside the tile gives every packet its pool offset (kept for pass 6), the bytes are copied
//                 by a 16-lane row per packet (sx_send_copy)
//     6. records  the destination tiles again: a scan inside the tile gives every packet its record index; the offsets are its source's
//
// A pool datagram is written iff it ends inside min(capacity, 2^31 - 1); record k is written iff k < max_records and its datagram was.
// Everything below compiles for the host as well (tests/test_shared_mix_model.py), through the same per-packet functions.
#pragma once
#include "solo_send.h"

#define SX_FAN_NOTHING (-1)     // SxSendPlan::why of a destination without a source: no datagram, and not counted either

struct SxFanArgs {
    const u8* bits; const i16* nbytes; const i32* source; const i32* dst_stream; const u8* send; const i32* seq_base;
    i32* named;                 // [n_src]: 1 = some destination names the row
    i64* pool_off;              // [n_src][n_packets]: where the packet's first datagram lies in the pool (valid packets of named rows)
    int n_src, n_dst, n_packets, slot, hbb;
    i32 first_seq;
};

// What the host refuses (solo_api.hip and the host form both ask here).
static inline bool sx_fan_args_ok(const void* bits, const void* nbytes, long long n_src, const void* source, long long n_dst, long long n_packets,
                                  const void* records, long long max_records, const void* payload, long long cap, const void* count) {
    if (!bits || !nbytes || !source || !records || !payload || !count) return false;
    if (n_src <= 0 || n_dst <= 0 || n_packets <= 0 || max_records < 0 || cap < 0) return false;
    return n_dst * n_packets * 2 < (1LL << 31) && n_src * n_packets * 2 < (1LL << 31);
}

// source packet q of the pool order (q = p * n_src + s) -> its index in the table, its plan with both descriptions (EMPTY for a row that
// nobody names: its length record is not read)
SX_HD SxSendPlan sx_fan_src_plan(const SxFanArgs& a, int q, size_t* pk) {
    const int p = q / a.n_src, s = q - p * a.n_src;
    *pk = (size_t)s * (size_t)a.n_packets + (size_t)p;
    if (!a.named[s]) return sx_send_no_plan(SX_SEND_EMPTY);
    return sx_send_plan(a.nbytes[*pk * 2 + 0], a.nbytes[*pk * 2 + 1], a.slot, a.hbb, 3, 0);
}
// destination packet q of the record order (q = p * n_dst + i) -> its stream, its source packet, its plan
SX_HD SxSendPlan sx_fan_dst_plan(const SxFanArgs& a, int q, int* stream, size_t* pk) {
    const int p = q / a.n_dst, i = q - p * a.n_dst;
    const i32 s = a.source[i];
    *stream = a.dst_stream ? a.dst_stream[i] : i;
    *pk = 0;
    if (s < 0) return sx_send_no_plan(SX_FAN_NOTHING);
    *pk = (size_t)s * (size_t)a.n_packets + (size_t)p;
    const long long seq = (long long)a.first_seq + (a.seq_base ? (long long)a.seq_base[i] : 0) + (long long)p;
    const int mask = a.send ? (int)a.send[(size_t)i * (size_t)a.n_packets + (size_t)p] & 3 : 3;
    return sx_send_plan(a.nbytes[*pk * 2 + 0], a.nbytes[*pk * 2 + 1], a.slot, a.hbb, mask, seq);
}
// the run of a source packet whose first datagram lies at `off`: what ends inside cap (both datagrams are neighbours in the slot and in the pool)
SX_HD SxSendRun sx_fan_run(const SxSendPlan& pl, size_t pk, int slot, i64 off, i64 cap) {
    SxSendRun run = sx_send_no_run();
    const bool w0 = pl.len0 > 0 && off + pl.len0 <= cap;
    const bool w1 = pl.len1 > 0 && off + pl.len0 + pl.len1 <= cap;
    if (w0 | w1) {
        run.src = (i64)(pk * (size_t)slot) + (w0 ? 0 : pl.src1);
        run.dst = (i32)(w0 ? off : off + pl.len0);
        run.len = (w0 ? pl.len0 : 0) + (w1 ? pl.len1 : 0);
    }
    return run;
}
// the records of a destination packet, the first of which has index k; off: the pool offset of its source packet -> records written
// (sx_send_record's rule; MD2 follows the source's MD1, sent or not)
SX_HD int sx_fan_emit(const SxSendPlan& pl, int stream, i32 k, i64 off, SxSendRecord* records, int max_records, i64 cap) {
    const bool w0 = sx_send_record(records, k, max_records, cap, stream, pl.seq, 0, off, pl.len0);
    const bool w1 = sx_send_record(records, k + (pl.len0 > 0), max_records, cap, stream, pl.seq, 1, off + pl.src1, pl.len1);
    return (int)w0 + (int)w1;
}

struct SxFanLayout { SxSendBase* bases; i32* totals; i32* named; i64* pool_off; int src_tiles, dst_tiles; };
static inline int sx_fan_tiles(int n, int n_packets) { return (n * n_packets + SX_SEND_TILE - 1) / SX_SEND_TILE; }
// bytes of device scratch a call needs: tile bases (16 bytes) | pool offsets | tile totals (two words) | the flags
static inline size_t solo_fan_scratch_bytes(int n_src, int n_dst, int n_packets) {
    const size_t tiles = (size_t)sx_fan_tiles(n_src, n_packets) + (size_t)sx_fan_tiles(n_dst, n_packets);
    return tiles * (sizeof(SxSendBase) + 2 * sizeof(i32)) + (size_t)n_src * (size_t)n_packets * sizeof(i64) + (size_t)n_src * sizeof(i32);
}
static inline SxFanLayout solo_fan_layout(void* scratch, int n_src, int n_dst, int n_packets) {
    SxFanLayout l;
    l.src_tiles = sx_fan_tiles(n_src, n_packets); l.dst_tiles = sx_fan_tiles(n_dst, n_packets);
    l.bases = (SxSendBase*)scratch;
    l.pool_off = (i64*)(l.bases + l.src_tiles + l.dst_tiles);
    l.totals = (i32*)(l.pool_off + (size_t)n_src * (size_t)n_packets);
    l.named = l.totals + 2 * (size_t)(l.src_tiles + l.dst_tiles);
    return l;
}

#if defined(__HIPCC__)
__global__ void __launch_bounds__(256) solo_fan_clear_kernel(i32* __restrict__ named, int n_src, u32* verdict) {
    const int s = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (s < n_src) named[s] = 0;
    if (s == 0) *verdict = 0;
}
__global__ void __launch_bounds__(256) solo_fan_mark_kernel(const i32* __restrict__ source, int n_dst, int n_src, i32* named, u32* verdict) {
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= n_dst) return;
    const i32 s = source[i];
    if (s < -1 || s >= n_src) atomicOr(verdict, 1u);
    else if (s >= 0) named[s] = 1;
}
// pass 3: totals[tile] = {counts (packed as sx_send_counts), bytes}; the source tiles come first
__global__ void __launch_bounds__(SX_SEND_TILE) solo_fan_totals_kernel(const SxFanArgs a, int src_tiles, i32* __restrict__ totals, const u32* verdict) {
    __shared__ i32 red[4];
    if (sx_map_refused(a.source, verdict)) return;
    const bool is_src = (int)blockIdx.x < src_tiles;
    const int q = ((int)blockIdx.x - (is_src ? 0 : src_tiles)) * SX_SEND_TILE + (int)threadIdx.x;
    i32 cnt = 0, bytes = 0;
    size_t pk;
    if (is_src) {
        if (q < a.n_src * a.n_packets) {
            const SxSendPlan pl = sx_fan_src_plan(a, q, &pk);
            bytes = pl.len0 + pl.len1;
        }
    } else if (q < a.n_dst * a.n_packets) {
        int stream;
        const SxSendPlan pl = sx_fan_dst_plan(a, q, &stream, &pk);
        cnt = sx_send_counts(pl);
    }
    cnt = wg_sum(cnt, red);
    bytes = wg_sum(bytes, red);
    if (threadIdx.x == 0) { totals[blockIdx.x * 2 + 0] = cnt; totals[blockIdx.x * 2 + 1] = bytes; }
}
// pass 4 is solo_send_scan_kernel (solo_send.h) over both runs of tile totals
// pass 5: the pool
__global__ void __launch_bounds__(SX_SEND_TILE) solo_fan_pool_kernel(const SxFanArgs a, const SxSendBase* __restrict__ bases, u8* __restrict__ payload,
                                                                     long long cap, SxSendCount* count, const u32* verdict) {
    __shared__ i32 red[4], part[1][4];
    __shared__ SxSendRun runs[SX_SEND_TILE];
    if (sx_map_refused(a.source, verdict)) return;
    const int tid = (int)threadIdx.x;
    const int q = (int)blockIdx.x * SX_SEND_TILE + tid;
    SxSendPlan pl = sx_send_no_plan(SX_SEND_EMPTY);
    size_t pk = 0;
    if (q < a.n_src * a.n_packets) pl = sx_fan_src_plan(a, q, &pk);
    const i32 bytes = pl.len0 + pl.len1;
    const i32 ibytes = wg_scan_incl(bytes, part);
    SxSendRun run = sx_send_no_run();
    if (bytes) {
        const i64 off = bases[blockIdx.x].bytes + (i64)(ibytes - bytes);
        a.pool_off[pk] = off;
        run = sx_fan_run(pl, pk, a.slot, off, cap);
    }
    runs[tid] = run;
    const i32 tile_bytes = wg_sum(run.len, red);                // (its barriers publish runs[])
    if (tid == 0 && tile_bytes) atomicAdd((unsigned long long*)&count->bytes, (unsigned long long)tile_bytes);
    sx_send_copy_runs(runs, payload, a.bits);
}
// pass 6: the records (bases: those of the destination tiles)
__global__ void __launch_bounds__(SX_SEND_TILE) solo_fan_records_kernel(const SxFanArgs a, const SxSendBase* __restrict__ bases, SxSendRecord* __restrict__ records,
                                                                        int max_records, long long cap, SxSendCount* count, const u32* verdict) {
    __shared__ i32 red[4], part[1][4];
    if (sx_map_refused(a.source, verdict)) return;
    const int tid = (int)threadIdx.x;
    const int q = (int)blockIdx.x * SX_SEND_TILE + tid;
    SxSendPlan pl = sx_send_no_plan(SX_FAN_NOTHING);
    int stream = 0; size_t pk = 0;
    if (q < a.n_dst * a.n_packets) pl = sx_fan_dst_plan(a, q, &stream, &pk);
    const i32 rec = (pl.len0 > 0) + (pl.len1 > 0);
    const i32 irec = wg_scan_incl(rec, part);
    int n_written = 0;
    if (rec) n_written = sx_fan_emit(pl, stream, bases[blockIdx.x].records + irec - rec, a.pool_off[pk], records, max_records, cap);
    const i32 tile_written = wg_sum(n_written, red);
    if (tid == 0 && tile_written) atomicAdd(&count->records, tile_written);
}

// (scratch: solo_fan_scratch_bytes(n_src, n_dst, n_packets) bytes, 16-byte aligned; a.named / a.pool_off are set here)
static inline hipError_t solo_fan_launch(SxFanArgs a, void* scratch, SxSendRecord* records, int max_records, u8* payload, long long cap, SxSendCount* count,
                                         u32* verdict, hipStream_t s) {
    const SxFanLayout l = solo_fan_layout(scratch, a.n_src, a.n_dst, a.n_packets);
    a.named = l.named; a.pool_off = l.pool_off;
    if (cap > 0x7FFFFFFFLL) cap = 0x7FFFFFFFLL;
    hipLaunchKernelGGL(solo_fan_clear_kernel, dim3((a.n_src + 255) / 256), dim3(256), 0, s, l.named, a.n_src, verdict);
    hipLaunchKernelGGL(solo_fan_mark_kernel, dim3((a.n_dst + 255) / 256), dim3(256), 0, s, a.source, a.n_dst, a.n_src, l.named, verdict);
    hipLaunchKernelGGL(solo_fan_totals_kernel, dim3(l.src_tiles + l.dst_tiles), dim3(SX_SEND_TILE), 0, s, a, l.src_tiles, l.totals, verdict);
    hipLaunchKernelGGL(solo_send_scan_kernel, dim3(1), dim3(64), 0, s, l.totals, l.bases, l.src_tiles + l.dst_tiles, count, a.source, verdict);
    hipLaunchKernelGGL(solo_fan_pool_kernel, dim3(l.src_tiles), dim3(SX_SEND_TILE), 0, s, a, l.bases, payload, cap, count, verdict);
    hipLaunchKernelGGL(solo_fan_records_kernel, dim3(l.dst_tiles), dim3(SX_SEND_TILE), 0, s, a, l.bases + l.src_tiles, records, max_records, cap, count, verdict);
    return hipGetLastError();
}
#else
// Host form of the passes (tests): packet by packet through the per-packet functions above.  -> false: refused "on the device", nothing
// but count->records = -1 is written
static inline bool sx_fan_host(SxFanArgs a, SxSendRecord* records, int max_records, u8* payload, long long cap, SxSendCount* count) {
    for (int i = 0; i < a.n_dst; i++)
        if (a.source[i] < -1 || a.source[i] >= a.n_src) { count->records = -1; return false; }
    if (cap > 0x7FFFFFFFLL) cap = 0x7FFFFFFFLL;
    const int n_sp = a.n_src * a.n_packets, n_dp = a.n_dst * a.n_packets;
    a.named = new i32[(size_t)a.n_src]();
    a.pool_off = new i64[(size_t)n_sp];
    for (int i = 0; i < a.n_dst; i++) if (a.source[i] >= 0) a.named[a.source[i]] = 1;
    SxSendCount c; c.records = 0; c.records_needed = 0; c.bytes = 0; c.bytes_needed = 0; c.empty = 0; c.refused = 0;
    for (int q = 0; q < n_sp; q++) {                        // pass 5 (its offsets are the running sum that passes 3 and 4 give it)
        size_t pk;
        const SxSendPlan pl = sx_fan_src_plan(a, q, &pk);
        if (pl.len0 + pl.len1 == 0) continue;
        a.pool_off[pk] = c.bytes_needed;
        const SxSendRun r = sx_fan_run(pl, pk, a.slot, c.bytes_needed, cap);
        for (int lane = 0; lane < SX_SEND_ROW && r.len > 0; lane++) sx_send_copy(payload + r.dst, a.bits + r.src, r.len, lane, SX_SEND_ROW);
        c.bytes += r.len;
        c.bytes_needed += pl.len0 + pl.len1;
    }
    for (int q = 0; q < n_dp; q++) {                        // pass 6
        int stream; size_t pk;
        const SxSendPlan pl = sx_fan_dst_plan(a, q, &stream, &pk);
        const i32 cnt = sx_send_counts(pl);
        c.empty += (cnt >> 10) & 1023; c.refused += (cnt >> 20) & 1023;
        if ((cnt & 1023) == 0) continue;
        c.records += sx_fan_emit(pl, stream, c.records_needed, a.pool_off[pk], records, max_records, cap);
        c.records_needed += cnt & 1023;
    }
    *count = c;
    delete[] a.named;
    delete[] a.pool_off;
    return true;
}
#endif

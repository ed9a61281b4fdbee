// solo_send.h -- the sender back end: the slots an encode call wrote -> the datagrams that go on the wire (solo_send_pack, include/solo_mi355x.h).
//
// solo_batch_encode leaves one fixed slot per packet (MD1 || MD2 || HB) and a length record {total, len(MD2) + HB}.  A packet travels as
// up to two datagrams (MD1, and MD2 || HB), so the send side is a stream compaction over n x P x 2 candidates with two running sums:
// records (one solo_arrival_t per datagram -- what solo_recv_insert of the receiving handle takes) and payload bytes (a dense pool in the
// same order).  The order is fixed -- packet-major (p outer), then row i, then description 0 before 1 -- so a tick's datagrams are
// contiguous and the output is a pure function of the inputs.  Three short launches, none of which waits for another workgroup:
//
//     1. totals   one workgroup per tile of SX_SEND_TILE packets (one lane per packet): {datagrams, bytes, empty, refused} of the tile
//     2. scan     ONE wavefront walks the tile totals 64 at a time (wv_scan_incl) -> every tile's first record index and byte offset,
//                 and the call's counts
//     3. scatter  the tile again: the same plan per packet, a scan inside the tile (wg_scan_incl, solo_wave.h), records written by the
//                 packet's lane, then the bytes: a 16-lane row per packet
//
// The length rules are ONE function (sx_send_plan) that passes 1 and 3 both call, so they cannot disagree.  A packet's payload is already
// contiguous in its slot, so with both descriptions sent its two datagrams are one run of `total` bytes in the pool; the run's source is
// wherever the slot puts it, its destination has any byte alignment: the copy stores aligned dwords, each funnelled out of the two aligned
// source dwords around it, and moves the up to three bytes at either edge one by one.  Nothing outside a run is read (a source dword that
// reaches over the run's ends is put together from its inside bytes) and nothing outside [0, capacity) or [0, max_records) is written.
//
// Everything below compiles for the host as well (tests/test_send_pack_model.py builds sx_send_pack_host, the three passes run tile by
// tile through the very per-packet functions of the kernels, and compares it with an independent model).
#pragma once
#include "solo_wave.h"
#include "solo_stream_ctl.h"
#include "../../include/solo_mi355x.h"

#define SX_SEND_TILE 256        // packets per tile = lanes per workgroup of passes 1 and 3
#define SX_SEND_ROW 16          // lanes that copy one packet's run (four packets per wavefront: a 78-byte packet is 20 dwords)

// what became of a packet
#define SX_SEND_OK 0
#define SX_SEND_EMPTY 1         // total <= 0: a DTX packet, nothing to send
#define SX_SEND_TOO_LARGE 2     // total > slot
#define SX_SEND_N1_NEGATIVE 3   // len(MD2) + HB < 0
#define SX_SEND_N1_OVER 4       // len(MD2) + HB > total
#define SX_SEND_N1_SHORT 5      // a second description shorter than the high-band bytes it ends with
#define SX_SEND_SEQ 6           // the sequence number is negative or does not fit int32

typedef solo_send_count_t SxSendCount;
static_assert(sizeof(SxSendCount) == 32, "solo_send_count_t layout");

typedef solo_arrival_t SxSendRecord;                        // what solo_recv_insert takes: SxRecvArrival of solo_recv.h
static_assert(sizeof(SxSendRecord) == 20, "solo_arrival_t layout");

struct SxSendPlan { i32 why, len0, len1, src1, seq; };      // len0 / len1: bytes of the MD1 / MD2 || HB datagram (0: none); src1: where MD2 starts in the slot
// a packet without a datagram, and why
SX_HD SxSendPlan sx_send_no_plan(i32 why) {
    SxSendPlan r;
    r.why = why; r.len0 = 0; r.len1 = 0; r.src1 = 0; r.seq = 0;
    return r;
}

// The length rules.  hbb: high-band bytes per packet (8; 4 with framesize_ms 20 or joint_mode 1), mask: bit 0 sends MD1, bit 1 MD2 || HB.
// An empty packet is empty whatever else is wrong with it; a record that fails a rule yields nothing and is never dereferenced.
SX_HD SxSendPlan sx_send_plan(i32 total, i32 n1, int slot, int hbb, int mask, long long seq) {
    SxSendPlan r = sx_send_no_plan(SX_SEND_OK);
    r.seq = (i32)seq;
    if (total <= 0) r.why = SX_SEND_EMPTY;
    else if (seq < 0 || seq > 0x7FFFFFFFLL) r.why = SX_SEND_SEQ;
    else if (total > slot) r.why = SX_SEND_TOO_LARGE;
    else if (n1 < 0) r.why = SX_SEND_N1_NEGATIVE;
    else if (n1 > total) r.why = SX_SEND_N1_OVER;
    else if (n1 > 0 && n1 < hbb) r.why = SX_SEND_N1_SHORT;
    if (r.why != SX_SEND_OK) return r;
    r.src1 = total - n1;
    if ((mask & 1) && total - n1 > 0) r.len0 = total - n1;
    if ((mask & 2) && n1 > hbb) r.len1 = n1;                // (n1 == hbb would be high-band bytes alone: the receiver drops such a datagram)
    return r;
}

struct SxSendArgs {
    const u8* bits; const i16* nbytes; const u8* send; const i32* seq_base; const i32* map;
    int n, n_packets, slot, hbb;
    i32 first_seq;
};

// packet q of the output order (q = p * n + i) -> its row, its record index in the caller's arrays, its plan
SX_HD SxSendPlan sx_send_packet(const SxSendArgs& a, int q, int* row, size_t* pk) {
    const int p = q / a.n, i = q - p * a.n;
    *row = i;
    *pk = (size_t)i * (size_t)a.n_packets + (size_t)p;
    const long long seq = (long long)a.first_seq + (a.seq_base ? (long long)a.seq_base[i] : 0) + (long long)p;
    return sx_send_plan(a.nbytes[*pk * 2 + 0], a.nbytes[*pk * 2 + 1], a.slot, a.hbb, a.send ? (int)a.send[*pk] & 3 : 3, seq);
}
// what a packet adds to the tile totals: datagrams | empty << 10 | refused << 20 (each at most SX_SEND_TILE x 2 per tile), and bytes
SX_HD i32 sx_send_counts(const SxSendPlan& pl) {
    return (pl.len0 > 0) + (pl.len1 > 0) + ((pl.why == SX_SEND_EMPTY) << 10) + ((pl.why > SX_SEND_EMPTY) << 20);
}

struct SxSendBase { i64 bytes; i32 records, pad; };         // where a tile's output starts
struct SxSendRun { i64 src; i32 dst, len; };                // bytes of one packet that pass 3 copies: bits[src ..) -> payload[dst ..)
SX_HD SxSendRun sx_send_no_run() {
    SxSendRun run;
    run.src = 0; run.dst = 0; run.len = 0;
    return run;
}

// THE record rule, of solo_send_pack and solo_send_fanout alike: record k, of description `desc`'s datagram of `len` bytes at pool offset
// `off`, is written iff there is such a datagram (len > 0), k < max_records and the datagram ends inside cap (<= 2^31 - 1: an offset that
// is written fits its int32 field).  -> written
SX_HD bool sx_send_record(SxSendRecord* records, i32 k, int max_records, i64 cap, int stream, i32 seq, i32 desc, i64 off, i32 len) {
    if (!(len > 0 && k < max_records && off + len <= cap)) return false;
    SxSendRecord r; r.stream = stream; r.seq = seq; r.desc = desc; r.offset = (i32)off; r.len = len;
    records[k] = r;
    return true;
}
// The packet's records, given the index k and the pool offset `off` of its first datagram.  Both sums grow along the order, so what is
// written is a prefix -- and a packet whose MD1 record is cut loses its MD2 record as well, so the written part of a packet is always ONE run.
SX_HD SxSendRun sx_send_emit(const SxSendPlan& pl, int stream, size_t pk, int slot, i32 k, i64 off, SxSendRecord* records, int max_records, i64 cap,
                             int* n_written) {
    SxSendRun run = sx_send_no_run();
    *n_written = 0;
    const i64 off1 = off + pl.len0;
    const bool w0 = sx_send_record(records, k, max_records, cap, stream, pl.seq, 0, off, pl.len0);
    const bool w1 = sx_send_record(records, k + (pl.len0 > 0), max_records, cap, stream, pl.seq, 1, off1, pl.len1);
    if (w0 | w1) {
        run.src = (i64)(pk * (size_t)slot) + (w0 ? 0 : pl.src1);
        run.dst = (i32)(w0 ? off : off1);
        run.len = (w0 ? pl.len0 : 0) + (w1 ? pl.len1 : 0);
        *n_written = (int)w0 + (int)w1;
    }
    return run;
}

// the aligned dword at `a`, of which only the bytes inside [lo, hi) are read (the others come out as 0)
SX_HD u32 sx_send_ld_clipped(const u8* a, const u8* lo, const u8* hi) {
    if (a >= lo && a + 4 <= hi) return *(const u32*)a;
    u32 v = 0;
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (a + k >= lo && a + k < hi) v |= (u32)a[k] << (8 * k);
    return v;
}
// dst[0 .. n) = src[0 .. n) by `nlanes` (>= 3) lanes, this one being `lane`: the destination's aligned dwords are stored whole, each
// funnelled (v_alignbyte_b32) out of the two aligned source dwords it straddles; the bytes in front of the first and behind the last
// aligned destination dword (at most three each) go one by one.
SX_HD void sx_send_copy(u8* dst, const u8* src, int n, int lane, int nlanes) {
    const int head = sx_min(n, (int)((0 - (uintptr_t)dst) & 3));
    const int body = (n - head) >> 2, tail = n - head - 4 * body;
    if (lane < head) dst[lane] = src[lane];
    if (lane < tail) dst[head + 4 * body + lane] = src[head + 4 * body + lane];
    const u32 sh = (u32)((uintptr_t)(src + head) & 3);
    const u8* sa = src + head - (int)sh;                    // (aligned; up to three bytes in front of the run, which are not read)
    u32* d32 = (u32*)(dst + head);
    for (int j = lane; j < body; j += nlanes) {
        u32 v = sx_send_ld_clipped(sa + 4 * j, src, src + n);
        if (sh) {
            const u32 up = sx_send_ld_clipped(sa + 4 * j + 4, src, src + n);
#if defined(__HIP_DEVICE_COMPILE__)
            v = __builtin_amdgcn_alignbyte(up, v, sh);
#else
            v = (v >> (8 * sh)) | (up << (32 - 8 * sh));
#endif
        }
        d32[j] = v;
    }
}

#if defined(__HIPCC__)
// the bytes of a tile, whose runs its lanes have left in runs[] (published by a barrier): a 16-lane row per packet
__device__ __forceinline__ void sx_send_copy_runs(const SxSendRun* runs, u8* payload, const u8* bits) {
    const int tid = (int)threadIdx.x, lane = tid & (SX_SEND_ROW - 1);
    for (int t = tid / SX_SEND_ROW; t < SX_SEND_TILE; t += SX_SEND_TILE / SX_SEND_ROW) {
        const SxSendRun r = runs[t];
        if (r.len > 0) sx_send_copy(payload + r.dst, bits + r.src, r.len, lane, SX_SEND_ROW);
    }
}

// pass 1: totals[tile] = {counts (packed as sx_send_counts), bytes}
__global__ void __launch_bounds__(SX_SEND_TILE) solo_send_totals_kernel(const SxSendArgs a, int n_pk, i32* __restrict__ totals, const u32* verdict) {
    __shared__ i32 red[4];
    if (sx_map_refused(a.map, verdict)) return;
    const int q = (int)blockIdx.x * SX_SEND_TILE + (int)threadIdx.x;
    i32 cnt = 0, bytes = 0;
    if (q < n_pk) {
        int row; size_t pk;
        const SxSendPlan pl = sx_send_packet(a, q, &row, &pk);
        cnt = sx_send_counts(pl);
        bytes = pl.len0 + pl.len1;
    }
    cnt = wg_sum(cnt, red);
    bytes = wg_sum(bytes, red);
    if (threadIdx.x == 0) { totals[blockIdx.x * 2 + 0] = cnt; totals[blockIdx.x * 2 + 1] = bytes; }
}

// pass 2, of solo_send_fanout (solo_fanout.h: its source and destination tiles in one run, map = its source rows) as well: one wavefront;
// a tile holds at most 2^23 bytes, so 64 of them scan in 32 bits and the running base is carried in 64
__global__ void __launch_bounds__(64) solo_send_scan_kernel(const i32* __restrict__ totals, SxSendBase* __restrict__ bases, int n_tiles, SxSendCount* count,
                                                            const i32* map, const u32* verdict) {
    if (sx_map_refused(map, verdict)) {
        if (threadIdx.x == 0) count->records = -1;
        return;
    }
    i64 byte_base = 0;
    i32 rec_base = 0, empty = 0, refused = 0;
    for (int t0 = 0; t0 < n_tiles; t0 += 64) {
        const int t = t0 + (int)threadIdx.x;
        const i32 cnt = t < n_tiles ? totals[t * 2 + 0] : 0, bytes = t < n_tiles ? totals[t * 2 + 1] : 0;
        const i32 rec = cnt & 1023;
        const i32 irec = wv_scan_incl(rec), ibytes = wv_scan_incl(bytes);
        if (t < n_tiles) {
            SxSendBase b; b.bytes = byte_base + (i64)(ibytes - bytes); b.records = rec_base + irec - rec; b.pad = 0;
            bases[t] = b;
        }
        rec_base += __builtin_amdgcn_readlane(irec, 63);
        byte_base += (i64)__builtin_amdgcn_readlane(ibytes, 63);
        empty += wv_sum((cnt >> 10) & 1023);
        refused += wv_sum((cnt >> 20) & 1023);
    }
    if (threadIdx.x == 0) {         // (records / bytes WRITTEN: the later passes add what each tile wrote)
        SxSendCount c; c.records = 0; c.records_needed = rec_base; c.bytes = 0; c.bytes_needed = byte_base; c.empty = empty; c.refused = refused;
        *count = c;
    }
}

// pass 3: records by the packet's lane, then the bytes by a 16-lane row per packet
__global__ void __launch_bounds__(SX_SEND_TILE) solo_send_scatter_kernel(const SxSendArgs a, int n_pk, const SxSendBase* __restrict__ bases,
                                                                        SxSendRecord* __restrict__ records, int max_records, u8* __restrict__ payload,
                                                                        long long cap, SxSendCount* count, const u32* verdict) {
    __shared__ i32 red[4], part[2][4];
    __shared__ SxSendRun runs[SX_SEND_TILE];
    if (sx_map_refused(a.map, verdict)) return;
    const int tid = (int)threadIdx.x;
    const int q = (int)blockIdx.x * SX_SEND_TILE + tid;
    SxSendPlan pl = sx_send_no_plan(SX_SEND_EMPTY);
    int row = 0; size_t pk = 0;
    if (q < n_pk) pl = sx_send_packet(a, q, &row, &pk);
    const i32 rec = (pl.len0 > 0) + (pl.len1 > 0), bytes = pl.len0 + pl.len1;
    i32 incl[2] = {rec, bytes};
    wg_scan_incl(incl, part);
    const SxSendBase base = bases[blockIdx.x];
    int n_written = 0;
    SxSendRun run = sx_send_no_run();
    if (rec) run = sx_send_emit(pl, a.map ? a.map[row] : row, pk, a.slot, base.records + incl[0] - rec, base.bytes + (i64)(incl[1] - bytes), records, max_records, cap, &n_written);
    runs[tid] = run;
    const i32 tile_written = wg_sum(n_written, red), tile_bytes = wg_sum(run.len, red);      // (its barriers publish runs[])
    if (tid == 0 && tile_written) {
        atomicAdd(&count->records, tile_written);
        atomicAdd((unsigned long long*)&count->bytes, (unsigned long long)tile_bytes);
    }
    sx_send_copy_runs(runs, payload, a.bits);
}

// bytes of device scratch a call over n_pk packets needs: the tile totals, then the tile bases
static inline size_t solo_send_scratch_bytes(int n_pk) {
    const size_t n_tiles = ((size_t)n_pk + SX_SEND_TILE - 1) / SX_SEND_TILE;
    return n_tiles * (2 * sizeof(i32) + sizeof(SxSendBase));
}
static inline hipError_t solo_send_launch(const SxSendArgs& a, void* scratch, SxSendRecord* records, int max_records, u8* payload, long long cap,
                                          SxSendCount* count, const u32* verdict, hipStream_t s) {
    const int n_pk = a.n * a.n_packets, n_tiles = (n_pk + SX_SEND_TILE - 1) / SX_SEND_TILE;
    SxSendBase* bases = (SxSendBase*)scratch;               // (16-byte records first: the scratch is aligned for them)
    i32* totals = (i32*)(bases + n_tiles);
    if (cap > 0x7FFFFFFFLL) cap = 0x7FFFFFFFLL;
    hipLaunchKernelGGL(solo_send_totals_kernel, dim3(n_tiles), dim3(SX_SEND_TILE), 0, s, a, n_pk, totals, verdict);
    hipLaunchKernelGGL(solo_send_scan_kernel, dim3(1), dim3(64), 0, s, totals, bases, n_tiles, count, a.map, verdict);
    hipLaunchKernelGGL(solo_send_scatter_kernel, dim3(n_tiles), dim3(SX_SEND_TILE), 0, s, a, n_pk, bases, records, max_records, payload, cap, count, verdict);
    return hipGetLastError();
}
#else
// Host form of the three passes (tests): tile by tile, lane by lane, through the per-packet functions above.
static inline void sx_send_pack_host(const SxSendArgs& a, SxSendRecord* records, int max_records, u8* payload, long long cap, SxSendCount* count) {
    const int n_pk = a.n * a.n_packets, n_tiles = (n_pk + SX_SEND_TILE - 1) / SX_SEND_TILE;
    if (cap > 0x7FFFFFFFLL) cap = 0x7FFFFFFFLL;
    i32* totals = new i32[(size_t)n_tiles * 2];
    SxSendBase* bases = new SxSendBase[(size_t)n_tiles];
    for (int t = 0; t < n_tiles; t++) {                     // pass 1
        i32 cnt = 0, bytes = 0;
        for (int q = t * SX_SEND_TILE; q < n_pk && q < (t + 1) * SX_SEND_TILE; q++) {
            int row; size_t pk;
            const SxSendPlan pl = sx_send_packet(a, q, &row, &pk);
            cnt += sx_send_counts(pl);
            bytes += pl.len0 + pl.len1;
        }
        totals[t * 2 + 0] = cnt; totals[t * 2 + 1] = bytes;
    }
    SxSendCount c; c.records = 0; c.records_needed = 0; c.bytes = 0; c.bytes_needed = 0; c.empty = 0; c.refused = 0;
    for (int t = 0; t < n_tiles; t++) {                     // pass 2
        bases[t].bytes = c.bytes_needed; bases[t].records = c.records_needed; bases[t].pad = 0;
        c.records_needed += totals[t * 2] & 1023; c.bytes_needed += totals[t * 2 + 1];
        c.empty += (totals[t * 2] >> 10) & 1023; c.refused += (totals[t * 2] >> 20) & 1023;
    }
    for (int t = 0; t < n_tiles; t++) {                     // pass 3
        i32 k = bases[t].records;
        i64 off = bases[t].bytes;
        for (int q = t * SX_SEND_TILE; q < n_pk && q < (t + 1) * SX_SEND_TILE; q++) {
            int row, n_written = 0; size_t pk;
            const SxSendPlan pl = sx_send_packet(a, q, &row, &pk);
            if (pl.len0 + pl.len1 == 0) continue;
            const SxSendRun r = sx_send_emit(pl, a.map ? a.map[row] : row, pk, a.slot, k, off, records, max_records, cap, &n_written);
            for (int lane = 0; lane < SX_SEND_ROW && r.len > 0; lane++) sx_send_copy(payload + r.dst, a.bits + r.src, r.len, lane, SX_SEND_ROW);
            c.records += n_written; c.bytes += r.len;
            k += (pl.len0 > 0) + (pl.len1 > 0); off += pl.len0 + pl.len1;
        }
    }
    *count = c;
    delete[] totals;
    delete[] bases;
}
#endif

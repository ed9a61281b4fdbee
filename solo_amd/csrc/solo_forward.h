// solo_forward.h -- the middle of a forwarding server's tick (solo_forward_levels, solo_forward_route; include/solo_mi355x.h): the arrivals
// solo_rtp_parse wrote -> one RFC 6464 level per row for solo_vad_select, and the selected speakers' datagrams -> records for every other
// member of their room, under per-room slots whose packet numbers stay continuous when the speaker behind a slot changes.  No payload
// byte moves and nothing is decoded: a record points at the arrival's bytes in the receive buffer, which solo_rtp_pack is then given as
// its pool.  A DUPLICATE DATAGRAM IS FORWARDED TWICE: there is no ring here, the receivers' rings drop it.
//
// Levels (stateless).  An arrival counts when its stream is inside [0, n_rows) and its desc is 0 or 1; its byte is level_in[i], or the
// default where that is 255 (255: none).  Three short launches:
//     1. clear    a lane per row: {min_seq = 0xFFFFFFFF, max_seq = -1, dgrams = 0, key = 255}
//     2. gather   a lane per datagram: atomic min (unsigned) / max / add on the row's three words, atomic min of the byte's KEY
//                 (byte & 127) << 1 | !(byte >> 7) on the fourth -- the loudest first, voiced before unvoiced
//     3. finish   a lane per row: the key back to its byte -> {sa, level, byte, 0} in the fourth word, d_sa_q8[row], d_level[row]
// An unsigned minimum that starts at 0xFFFFFFFF leaves min_seq = -1 for a row without arrivals, and key 255 is byte 0x7F, "no level".
//
// Route.  The state is one SxFwdSlot {src, delta, start, next} per room and slot (solo_rows.h: a "row" of the object is a room).  Behind
// the room plan of solo_mix.h (clear, check, scan, scatter; a room id outside [-1, n_rooms) sets its verdict word and every kernel below
// leaves before it touches anything but the two refusal marks):
//     5. begin    one lane: the counts to zero, or the refusal marks
//     6. rooms    ONE wavefront per room (sx_fwd_room): the slots in registers; a slot whose source is no longer a selected member of the
//                 room becomes free; then the members pass by in INCREASING ROW ORDER, 64 at a time -- a room of at most 64 is ranked
//                 inside the wave (the plan's lists come in the order of its atomics), a larger one walks d_room itself, n / 64 steps --,
//                 each chunk writes its part of the sorted list and every member's rank, and a ballot of the selected members that hold
//                 no slot and have a datagram hands them the free slots, lowest row to lowest slot; then `next` of every slot moves
//                 behind its source's largest packet number, and the state and d_slot_src are written
//     7. verdicts a lane per arrival (sx_fwd_verdict): the first rule that fails, the fan-out (members - 1) of a forwarded one, its slot
//                 and packet number; an inclusive scan of the fan-outs inside the tile of 256, the tile's total, the counters;
//                 the same grid writes d_level_fwd, a lane per row
//     8. scan     ONE wavefront walks the tile totals 64 at a time -> every tile's first record, the call's records
//     9. emit     THE HOT PATH: a lane per OUTPUT record -- a binary search of its tile in the bases, of its arrival in the tile's scan,
//                 the t-th member of the room that is not the sender from the sorted list and the sender's rank -- writes one 20-byte
//                 record.  One arrival into a room of 4096 is 4095 lanes, not a loop
// Only commutative atomics (min, max, add on counters) are used: every output and the state are a pure function of inputs and state, and
// but for the order of the records, which follows the arrivals by definition, independent of the order of the arrivals.
//
// Everything outside the kernels compiles for the host as well (tests/test_forward_model.py builds sx_fwd_levels_host and
// sx_fwd_route_host: the passes run through the very functions of the kernels, with the 1-lane forms of solo_wave.h, and are compared with
// the independent model of tests/forward_model.py).
#pragma once
#include "solo_mix.h"
#include "solo_send.h"

#define SX_FWD_TILE 256             // arrivals, rows or records per workgroup
#define SX_FWD_MAX_SLOTS 8
#define SX_FWD_AHEAD 4              // chunks of d_room a large room's wavefront has in flight
#define SX_FWD_NO_LEVEL 0x7Fu       // the byte of a row or slot that has none: unvoiced, -127 dBov
#define SX_FWD_SEQ_MAX 0x7FFFFFFFLL

typedef solo_forward_row_t SxFwdRow;
static_assert(sizeof(SxFwdRow) == 16, "solo_forward_row_t layout");
typedef solo_forward_count_t SxFwdCount;
static_assert(sizeof(SxFwdCount) == 32, "solo_forward_count_t layout");
struct SxFwdSlot { i32 src, delta, start, next; };           // a room's slot: who it carries, seq -> packet number, the first and the next number
static_assert(sizeof(SxFwdSlot) == SOLO_FORWARD_STATE_BYTES(1), "a slot of the state");
#define SX_FWD_SLOT_WORDS 4

// what became of an arrival: the FIRST rule that fails, in this order (== the fields of solo_forward_count_t)
#define SX_FWD_FORWARDED 0
#define SX_FWD_REJECTED 1
#define SX_FWD_NO_DESC 2
#define SX_FWD_NO_ROOM 3
#define SX_FWD_NOT_SELECTED 4
#define SX_FWD_NO_SLOT 5
#define SX_FWD_STALE 6
#define SX_FWD_SWITCHES 7           // (the eighth counter: slots that took a new source)

// the record a reset leaves, word w of a room's state
static inline i32 sx_fwd_init_word(int w) { return (w % SX_FWD_SLOT_WORDS) == 0 ? -1 : 0; }

// ---- levels ------------------------------------------------------------------------------------------------------------------------
struct SxFwdLevelArgs {
    const SxSendRecord* arrivals; const u8* level_in;        // [n_dgrams]; level_in NULL = every datagram has the default
    SxFwdRow* rowinfo; u8* sa; u8* level;                    // [n_rows]
    int n_dgrams, n_rows, default_level;
};
SX_HD bool sx_fwd_levels_ok(const void* arrivals, int n_dgrams, int n_rows, int default_level, const void* rowinfo, const void* sa, const void* level) {
    return rowinfo && sa && level && n_dgrams >= 0 && (n_dgrams == 0 || arrivals) && n_rows > 0 && default_level >= 0 && default_level <= 255 &&
           !(((uintptr_t)rowinfo | (uintptr_t)arrivals) & 3);
}
SX_HD u32 sx_fwd_key(u32 byte) { return ((byte & 127u) << 1) | ((byte >> 7) ^ 1u); }
SX_HD u32 sx_fwd_key_byte(u32 key) { return (key >> 1) | (((key & 1u) ^ 1u) << 7); }
// does arrival r count for a call over n rows?
SX_HD bool sx_fwd_counts(const SxSendRecord& r, int n) { return r.stream >= 0 && r.stream < n && (r.desc == 0 || r.desc == 1); }
// the byte of datagram i; 255: none
SX_HD u32 sx_fwd_byte(const SxFwdLevelArgs& a, int i) {
    const u32 b = a.level_in ? (u32)a.level_in[i] : 255u;
    return b == 255u ? (u32)a.default_level : b;
}
// the four words of a row while a call gathers
SX_HD void sx_fwd_row_clear(u32* w) { w[0] = 0xFFFFFFFFu; w[1] = 0xFFFFFFFFu; w[2] = 0; w[3] = 255u; }
// ... and what the finish makes of the fourth: sa | level << 8 | byte << 16
SX_HD void sx_fwd_row_finish(const SxFwdLevelArgs& a, int s) {
    u32* w = (u32*)&a.rowinfo[s];
    const u32 byte = sx_fwd_key_byte(w[3] & 255u), sa = (byte & 128u) ? 255u : 0u, lv = byte & 127u;
    w[3] = sa | (lv << 8) | (byte << 16);
    a.sa[s] = (u8)sa; a.level[s] = (u8)lv;
}

// ---- route -------------------------------------------------------------------------------------------------------------------------
struct SxFwdArgs {
    const SxSendRecord* arrivals; const SxFwdRow* rowinfo; const u8* sel; const i32* room;
    SxFwdSlot* state;                                        // [n_rooms][K] of the object's [n_rows][K]
    i32* counts; i32* starts; i32* members; i32* rank;       // the room plan (solo_mix.h), its lists sorted by the rooms pass; rank [n]: a row's place in its list
    i32* a_incl; i32* a_q; i32* a_k;                         // [n_dgrams]: fan-outs scanned inside the tile, packet number, slot
    i32* totals; i32* bases;                                 // [tiles of arrivals]
    SxSendRecord* records; SxSendCount* send_count; u8* level_fwd; i32* slot_src; SxFwdCount* count;
    int n_dgrams, n, n_rooms, K, max_records;
};
static inline bool sx_fwd_route_ok(const void* f, int n_rows, const void* arrivals, int n_dgrams, const void* rowinfo, const void* sel, const void* room, int n,
                                   int n_rooms, const void* records, int max_records, const void* send_count, const void* slot_src, const void* count) {
    if (!f || !rowinfo || !sel || !room || !records || !send_count || !count) return false;
    if (n <= 0 || n > n_rows || n_rooms <= 0 || n_rooms > n_rows || n_dgrams < 0 || (n_dgrams > 0 && !arrivals) || max_records < 0) return false;
    if ((i64)n_dgrams * (i64)(n - 1) >= ((i64)1 << 31)) return false;
    if (((uintptr_t)arrivals | (uintptr_t)rowinfo | (uintptr_t)room | (uintptr_t)records | (uintptr_t)slot_src | (uintptr_t)count) & 3) return false;
    return !((uintptr_t)send_count & 7);
}
// bytes of scratch that depend on the object's rows: the room plan | rank
static inline size_t solo_forward_plan_bytes(int n_rows) { return sx_room_plan_bytes(n_rows) + (size_t)n_rows * sizeof(i32); }
// ... and on the arrivals of a call: a_incl | a_q | a_k | totals | bases
static inline size_t solo_forward_scratch_bytes(int n_dgrams) {
    const size_t n_tiles = ((size_t)n_dgrams + SX_FWD_TILE - 1) / SX_FWD_TILE;
    return (3 * (size_t)n_dgrams + 2 * n_tiles) * sizeof(i32);
}
static inline void sx_fwd_carve(SxFwdArgs& a, void* plan, int n_rows, void* scratch) {
    const SxRoomPlan rp = sx_room_plan(plan, n_rows);
    a.counts = rp.counts; a.starts = rp.starts; a.members = rp.members; a.rank = sx_room_plan_end(rp, n_rows);
    const size_t n_tiles = ((size_t)a.n_dgrams + SX_FWD_TILE - 1) / SX_FWD_TILE;
    a.a_incl = (i32*)scratch; a.a_q = a.a_incl + a.n_dgrams; a.a_k = a.a_q + a.n_dgrams; a.totals = a.a_k + a.n_dgrams; a.bases = a.totals + n_tiles;
}

// the lanes for which p holds, bit l = lane l; the set bits below this lane
SX_HD u64 sx_fwd_ballot(bool p) {
#if defined(__HIP_DEVICE_COMPILE__) && SX_NLANES == 64
    return (u64)__ballot(p);
#else
    return p ? 1u : 0u;
#endif
}
SX_HD int sx_fwd_popc(u64 m) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __popcll(m);
#else
    return __builtin_popcountll(m);
#endif
}
SX_HD int sx_fwd_below(u64 m) { return sx_fwd_popc(m & (((u64)1 << SX_LANE) - 1)); }
SX_HD int sx_fwd_first(u64 m) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __ffsll((unsigned long long)m) - 1;
#else
    return __builtin_ctzll(m);
#endif
}
// A list of m <= SX_NLANES distinct rows -> in increasing order, lane l gets the l-th (-1 beyond m): every lane counts the rows below
// its own, tmp (SX_NLANES words of LDS) turns the ranks into places
SX_HD i32 sx_fwd_sorted(const i32* mem, int m, i32* tmp) {
    const i32 x = SX_LANE < m ? mem[SX_LANE] : 0x7FFFFFFF;
    i32 rk = 0;
    for (int t = 0; t < m; t++) rk += sx_mix_lane(x, t) < x;
    if (SX_LANE < m) tmp[rk] = x;
    wv_sync();
    return SX_LANE < m ? tmp[SX_LANE] : -1;
}

// One room: what one wavefront does (the header of this file, pass 6) -> the slots that took a new source, in every lane
SX_HD i32 sx_fwd_room(const SxFwdArgs& a, int r, i32* tmp) {
    const int m = SX_UNI(a.counts[r]), first = SX_UNI(a.starts[r]), K = a.K;
    SxFwdSlot sl[SX_FWD_MAX_SLOTS];
    i32 n_free = 0, switches = 0;
    // step 1: a slot keeps a source that is still a selected member of this room
#pragma unroll
    for (int k = 0; k < SX_FWD_MAX_SLOTS; k++) {
        sl[k].src = -1; sl[k].delta = 0; sl[k].start = 0; sl[k].next = 0;
        if (k < K) {
            sl[k] = a.state[(size_t)r * K + k];
            const i32 x = SX_UNI(sl[k].src);
            const bool keeps = x >= 0 && x < a.n && a.room[x] == r && a.sel[x] != 0;
            sl[k].src = keeps ? x : -1;
            n_free += !keeps;
        }
    }
    // step 2: the members in increasing row order, a chunk of SX_NLANES at a time
    i32 seen = 0;
    // what a chunk does: this lane's member `row` of it (-1: none), the chunks in increasing row order
    auto chunk = [&](i32 row) {
        const u64 in = sx_fwd_ballot(row >= 0);
        if (row >= 0) {
            const i32 at = seen + sx_fwd_below(in);
            a.members[first + at] = row;
            a.rank[row] = at;
        }
        seen += sx_fwd_popc(in);
        bool cand = row >= 0 && n_free > 0 && a.sel[row] != 0 && a.rowinfo[row].dgrams > 0;
#pragma unroll
        for (int k = 0; k < SX_FWD_MAX_SLOTS; k++) cand = cand && row != sl[k].src;
        u64 cm = sx_fwd_ballot(cand);
        while (cm != 0 && n_free > 0) {
            const int t = sx_fwd_first(cm);
            cm &= cm - 1;
            const i32 x = sx_mix_lane(row, t);
            const i32 min_seq = SX_UNI(a.rowinfo[x].min_seq);
            bool taken = false;
#pragma unroll
            for (int k = 0; k < SX_FWD_MAX_SLOTS; k++)
                if (k < K && !taken && sl[k].src < 0) {
                    sl[k].src = x; sl[k].start = sl[k].next; sl[k].delta = sl[k].next - min_seq;
                    taken = true;
                }
            n_free--; switches++;
        }
    };
    if (m <= SX_NLANES) {
        if (m > 0) chunk(sx_fwd_sorted(a.members + first, m, tmp));
    } else {
        // (the room ids of SX_FWD_AHEAD chunks are requested before the first of them is used: a chunk is one dependent round trip otherwise)
        for (int c0 = 0; c0 < a.n; c0 += SX_FWD_AHEAD * SX_NLANES) {
            i32 id[SX_FWD_AHEAD];
#pragma unroll
            for (int u = 0; u < SX_FWD_AHEAD; u++) {
                const int i = c0 + u * SX_NLANES + SX_LANE;
                id[u] = i < a.n ? a.room[i] : -1;
            }
#pragma unroll
            for (int u = 0; u < SX_FWD_AHEAD; u++) chunk(id[u] == r ? c0 + u * SX_NLANES + SX_LANE : -1);
        }
    }
    // step 4: next behind the source's largest packet number; the state and who each slot carries
#pragma unroll
    for (int k = 0; k < SX_FWD_MAX_SLOTS; k++)
        if (k < K) {
            if (sl[k].src >= 0) {
                const i64 v = (i64)SX_UNI(a.rowinfo[sl[k].src].max_seq) + (i64)sl[k].delta + 1;
                if (v >= (i64)sl[k].start + 1 && v <= SX_FWD_SEQ_MAX && v > (i64)sl[k].next) sl[k].next = (i32)v;
            }
            if (SX_LANE == 0) {
                a.state[(size_t)r * K + k] = sl[k];
                if (a.slot_src) a.slot_src[(size_t)r * K + k] = sl[k].src;
            }
        }
    return switches;
}

// THE arrival rule: arrival i -> its verdict; for a forwarded one its fan-out, slot and packet number
struct SxFwdVerdict { i32 verdict, fan, k, q; };
SX_HD SxFwdVerdict sx_fwd_verdict(const SxFwdArgs& a, int i) {
    const SxSendRecord r = a.arrivals[i];
    SxFwdVerdict v; v.fan = 0; v.k = -1; v.q = 0;
    if (r.stream < 0 || r.stream >= a.n) { v.verdict = SX_FWD_REJECTED; return v; }
    if (r.desc != 0 && r.desc != 1) { v.verdict = SX_FWD_NO_DESC; return v; }
    const i32 room = a.room[r.stream];
    if (room < 0) { v.verdict = SX_FWD_NO_ROOM; return v; }
    if (a.sel[r.stream] == 0) { v.verdict = SX_FWD_NOT_SELECTED; return v; }
    i32 delta = 0, start = 0;
    for (int k = 0; k < a.K; k++) {
        const SxFwdSlot s = a.state[(size_t)room * a.K + k];
        if (s.src == r.stream) { v.k = k; delta = s.delta; start = s.start; }
    }
    if (v.k < 0) { v.verdict = SX_FWD_NO_SLOT; return v; }
    const i64 q = (i64)r.seq + (i64)delta;
    if (q < (i64)start || q > SX_FWD_SEQ_MAX - 1) { v.verdict = SX_FWD_STALE; return v; }
    v.verdict = SX_FWD_FORWARDED; v.fan = a.counts[room] - 1; v.q = (i32)q;
    return v;
}
// row m's bytes of d_level_fwd: its room's slots
SX_HD void sx_fwd_level_row(const SxFwdArgs& a, int m) {
    const i32 room = a.room[m];
    if (room < 0) return;
    for (int k = 0; k < a.K; k++) {
        const i32 src = a.state[(size_t)room * a.K + k].src;
        a.level_fwd[(size_t)m * a.K + k] = src >= 0 ? a.rowinfo[src].byte : (u8)SX_FWD_NO_LEVEL;
    }
}
// the records of the call (written by the scan): what the emission walks
SX_HD i32 sx_fwd_n_records(const SxFwdArgs& a) { return a.send_count->records; }
// THE record rule: output record j (< the call's records) -> its bytes; n_tiles tiles of arrivals
SX_HD i32 sx_fwd_emit(const SxFwdArgs& a, int n_tiles, i32 j) {
    int lo = 0, hi = n_tiles - 1;                            // the last tile whose first record is at or below j
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.bases[mid] <= j) lo = mid;
        else hi = mid - 1;
    }
    const i32 jj = j - a.bases[lo];
    const int i0 = lo * SX_FWD_TILE;
    int il = i0, ih = sx_min(i0 + SX_FWD_TILE, a.n_dgrams) - 1;     // the first arrival of the tile whose scan is above jj
    while (il < ih) {
        const int mid = (il + ih) >> 1;
        if (a.a_incl[mid] > jj) ih = mid;
        else il = mid + 1;
    }
    const SxSendRecord src = a.arrivals[il];
    const i32 t = jj - (il > i0 ? a.a_incl[il - 1] : 0);     // the t-th member that is not the sender
    const i32 room = a.room[src.stream];
    const i32 m = a.members[a.starts[room] + t + (t >= a.rank[src.stream])];
    SxSendRecord o; o.stream = m * a.K + a.a_k[il]; o.seq = a.a_q[il]; o.desc = src.desc; o.offset = src.offset; o.len = src.len;
    a.records[j] = o;
    return src.len;
}

#if defined(__HIPCC__)
__global__ void __launch_bounds__(SX_FWD_TILE) solo_forward_levels_clear_kernel(const SxFwdLevelArgs a) {
    const int s = (int)blockIdx.x * SX_FWD_TILE + (int)threadIdx.x;
    if (s < a.n_rows) sx_fwd_row_clear((u32*)&a.rowinfo[s]);
}
__global__ void __launch_bounds__(SX_FWD_TILE) solo_forward_levels_kernel(const SxFwdLevelArgs a) {
    const int i = (int)blockIdx.x * SX_FWD_TILE + (int)threadIdx.x;
    if (i >= a.n_dgrams) return;
    const SxSendRecord r = a.arrivals[i];
    if (!sx_fwd_counts(r, a.n_rows)) return;
    u32* w = (u32*)&a.rowinfo[r.stream];
    atomicMin(&w[0], (u32)r.seq);
    atomicMax((i32*)&w[1], r.seq);
    atomicAdd(&w[2], 1u);
    const u32 b = sx_fwd_byte(a, i);
    if (b != 255u) atomicMin(&w[3], sx_fwd_key(b));
}
__global__ void __launch_bounds__(SX_FWD_TILE) solo_forward_levels_finish_kernel(const SxFwdLevelArgs a) {
    const int s = (int)blockIdx.x * SX_FWD_TILE + (int)threadIdx.x;
    if (s < a.n_rows) sx_fwd_row_finish(a, s);
}
static inline hipError_t solo_forward_levels_launch(const SxFwdLevelArgs& a, hipStream_t s) {
    const unsigned row_tiles = (unsigned)((a.n_rows + SX_FWD_TILE - 1) / SX_FWD_TILE);
    hipLaunchKernelGGL(solo_forward_levels_clear_kernel, dim3(row_tiles), dim3(SX_FWD_TILE), 0, s, a);
    if (a.n_dgrams > 0)
        hipLaunchKernelGGL(solo_forward_levels_kernel, dim3((unsigned)((a.n_dgrams + SX_FWD_TILE - 1) / SX_FWD_TILE)), dim3(SX_FWD_TILE), 0, s, a);
    hipLaunchKernelGGL(solo_forward_levels_finish_kernel, dim3(row_tiles), dim3(SX_FWD_TILE), 0, s, a);
    return hipGetLastError();
}

// pass 5: the counts to zero (the later passes add to them), or the two marks of a refused call
__global__ void __launch_bounds__(64) solo_forward_begin_kernel(const SxFwdArgs a, const u32* verdict) {
    if (sx_map_refused(a.room, verdict)) {
        if (threadIdx.x == 0) { a.count->forwarded = -1; a.send_count->records = -1; }
        return;
    }
    if (threadIdx.x < 8) ((i32*)a.count)[threadIdx.x] = 0;
    if (threadIdx.x == 0) {
        SxSendCount c; c.records = 0; c.records_needed = 0; c.bytes = 0; c.bytes_needed = 0; c.empty = 0; c.refused = 0;
        *a.send_count = c;
    }
}
// pass 6: one wavefront per room
__global__ void __launch_bounds__(64) solo_forward_rooms_kernel(const SxFwdArgs a, const u32* verdict) {
    __shared__ i32 tmp[64];
    if (sx_map_refused(a.room, verdict)) return;
    const i32 switches = sx_fwd_room(a, (int)blockIdx.x, tmp);
    if (threadIdx.x == 0 && switches) atomicAdd(&a.count->switches, switches);
}
// pass 7: a lane per arrival, and a lane per row for d_level_fwd
__global__ void __launch_bounds__(SX_FWD_TILE) solo_forward_verdicts_kernel(const SxFwdArgs a, int n_tiles, const u32* verdict) {
    __shared__ i32 cnt[8], part[1][4];
    if (sx_map_refused(a.room, verdict)) return;
    const int tid = (int)threadIdx.x, i = (int)blockIdx.x * SX_FWD_TILE + tid;
    if (tid < 8) cnt[tid] = 0;
    __syncthreads();
    if (a.level_fwd && i < a.n) sx_fwd_level_row(a, i);
    if ((int)blockIdx.x >= n_tiles) return;                  // (the whole workgroup: rows beyond the arrivals)
    SxFwdVerdict v; v.verdict = -1; v.fan = 0; v.k = -1; v.q = 0;
    i64 bytes = 0;
    if (i < a.n_dgrams) {
        v = sx_fwd_verdict(a, i);
        atomicAdd(&cnt[v.verdict], 1);
        a.a_q[i] = v.q; a.a_k[i] = v.k;
        bytes = (i64)v.fan * (i64)a.arrivals[i].len;
    }
    const i32 incl = wg_scan_incl(v.fan, part);              // (its barrier publishes cnt[])
    if (i < a.n_dgrams) a.a_incl[i] = incl;
    bytes = wv_sum64(bytes);
    if ((tid & 63) == 0 && bytes) atomicAdd((unsigned long long*)&a.send_count->bytes_needed, (unsigned long long)bytes);
    if (tid == 0) a.totals[blockIdx.x] = wg_total(part[0]);
    if (tid < 7 && cnt[tid]) atomicAdd(&((i32*)a.count)[tid], cnt[tid]);
}
// pass 8: one wavefront; the records of a call stay below 2^31 (the host's check), so everything scans in 32 bits
__global__ void __launch_bounds__(64) solo_forward_scan_kernel(const SxFwdArgs a, int n_tiles, const u32* verdict) {
    if (sx_map_refused(a.room, verdict)) return;
    i32 base = 0;
    for (int t0 = 0; t0 < n_tiles; t0 += 64) {
        const int t = t0 + (int)threadIdx.x;
        const i32 tot = t < n_tiles ? a.totals[t] : 0;
        const i32 incl = wv_scan_incl(tot);
        if (t < n_tiles) a.bases[t] = base + incl - tot;
        base += __builtin_amdgcn_readlane(incl, 63);
    }
    if (threadIdx.x == 0) { a.send_count->records_needed = base; a.send_count->records = sx_min(base, a.max_records); }
}
// pass 9: a lane per output record
__global__ void __launch_bounds__(SX_FWD_TILE) solo_forward_emit_kernel(const SxFwdArgs a, int n_tiles, const u32* verdict) {
    if (sx_map_refused(a.room, verdict)) return;
    const i32 n = sx_fwd_n_records(a);
    const i32 j = (i32)blockIdx.x * SX_FWD_TILE + (i32)threadIdx.x;
    if ((i32)blockIdx.x * SX_FWD_TILE >= n) return;
    i64 bytes = 0;
    if (j < n) bytes = sx_fwd_emit(a, n_tiles, j);
    bytes = wv_sum64(bytes);
    if ((threadIdx.x & 63) == 0 && bytes) atomicAdd((unsigned long long*)&a.send_count->bytes, (unsigned long long)bytes);
}

// plan: solo_forward_plan_bytes(n_rows) bytes, scratch: solo_forward_scratch_bytes(n_dgrams) bytes; a.state, the inputs and the outputs set
static inline hipError_t solo_forward_route_launch(SxFwdArgs a, void* plan, int n_rows, void* scratch, u32* verdict, hipStream_t s) {
    sx_fwd_carve(a, plan, n_rows, scratch);
    const SxRoomPlan rp = sx_room_plan(plan, n_rows);
    const int n_tiles = (a.n_dgrams + SX_FWD_TILE - 1) / SX_FWD_TILE, row_tiles = (a.n + SX_FWD_TILE - 1) / SX_FWD_TILE;
    sx_room_plan_launch(rp, a.room, a.n, a.n_rooms, NULL, verdict, [](u32*) {}, s);
    hipLaunchKernelGGL(solo_forward_begin_kernel, dim3(1), dim3(64), 0, s, a, verdict);
    hipLaunchKernelGGL(solo_forward_rooms_kernel, dim3((unsigned)a.n_rooms), dim3(64), 0, s, a, verdict);
    hipLaunchKernelGGL(solo_forward_verdicts_kernel, dim3((unsigned)sx_max(n_tiles, row_tiles)), dim3(SX_FWD_TILE), 0, s, a, n_tiles, verdict);
    hipLaunchKernelGGL(solo_forward_scan_kernel, dim3(1), dim3(64), 0, s, a, n_tiles, verdict);
    if (a.max_records > 0 && n_tiles > 0) {
        const i64 most = sx_min((i64)a.max_records, (i64)a.n_dgrams * (i64)(a.n - 1));
        if (most > 0)
            hipLaunchKernelGGL(solo_forward_emit_kernel, dim3((unsigned)((most + SX_FWD_TILE - 1) / SX_FWD_TILE)), dim3(SX_FWD_TILE), 0, s, a, n_tiles, verdict);
    }
    return hipGetLastError();
}
#else
// Host form of the launches (tests): the same passes, through the functions above
static inline void sx_fwd_levels_host(const SxFwdLevelArgs& a) {
    for (int s = 0; s < a.n_rows; s++) sx_fwd_row_clear((u32*)&a.rowinfo[s]);
    for (int i = 0; i < a.n_dgrams; i++) {
        const SxSendRecord r = a.arrivals[i];
        if (!sx_fwd_counts(r, a.n_rows)) continue;
        u32* w = (u32*)&a.rowinfo[r.stream];
        if ((u32)r.seq < w[0]) w[0] = (u32)r.seq;           // (unsigned, as the atomic minimum)
        if (r.seq > (i32)w[1]) w[1] = (u32)r.seq;
        w[2]++;
        const u32 b = sx_fwd_byte(a, i);
        if (b != 255u && sx_fwd_key(b) < w[3]) w[3] = sx_fwd_key(b);
    }
    for (int s = 0; s < a.n_rows; s++) sx_fwd_row_finish(a, s);
}
// a.state: the object's records.  -> false: a room id outside [-1, n_rooms); the two marks are written and nothing else
static inline bool sx_fwd_route_host(SxFwdArgs a, int n_rows) {
    for (int i = 0; i < a.n; i++)
        if (a.room[i] < -1 || a.room[i] >= a.n_rooms) {
            a.count->forwarded = -1; a.send_count->records = -1;
            return false;
        }
    std::vector<i32> plan(solo_forward_plan_bytes(n_rows) / sizeof(i32), 0), scratch(solo_forward_scratch_bytes(a.n_dgrams) / sizeof(i32) + 1, 0);
    sx_fwd_carve(a, plan.data(), n_rows, scratch.data());
    const SxRoomPlan rp = sx_room_plan(plan.data(), n_rows);
    i32 rows, rooms;
    sx_room_plan_host(rp, a.room, a.n, a.n_rooms, &rows, &rooms);
    i32 c[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tmp[SX_NLANES];
    SxSendCount sc; sc.records = 0; sc.records_needed = 0; sc.bytes = 0; sc.bytes_needed = 0; sc.empty = 0; sc.refused = 0;
    for (int r = 0; r < a.n_rooms; r++) c[SX_FWD_SWITCHES] += sx_fwd_room(a, r, tmp);
    if (a.level_fwd)
        for (int m = 0; m < a.n; m++) sx_fwd_level_row(a, m);
    const int n_tiles = (a.n_dgrams + SX_FWD_TILE - 1) / SX_FWD_TILE;
    for (int t = 0; t < n_tiles; t++) {                     // pass 7
        i32 incl = 0;
        for (int i = t * SX_FWD_TILE; i < a.n_dgrams && i < (t + 1) * SX_FWD_TILE; i++) {
            const SxFwdVerdict v = sx_fwd_verdict(a, i);
            c[v.verdict]++;
            a.a_q[i] = v.q; a.a_k[i] = v.k;
            incl += v.fan;
            a.a_incl[i] = incl;
            sc.bytes_needed += (i64)v.fan * (i64)a.arrivals[i].len;
        }
        a.totals[t] = incl;
    }
    for (int t = 0; t < n_tiles; t++) { a.bases[t] = sc.records_needed; sc.records_needed += a.totals[t]; }        // pass 8
    sc.records = sx_min(sc.records_needed, a.max_records);
    *a.send_count = sc;
    for (i32 j = 0; j < sc.records; j++) a.send_count->bytes += sx_fwd_emit(a, n_tiles, j);                       // pass 9
    memcpy(a.count, c, sizeof(*a.count));
    return true;
}
#endif

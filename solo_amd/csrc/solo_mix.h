// solo_mix.h -- the conference bridge between the two halves of a media server: decoded PCM rows -> mix-minus PCM rows (solo_mix,
// include/solo_mi355x.h).  Row i sits in room d_room[i] (or in none); every member of a room hears the sum of the others.
//
//     c_j[s]   = (x_j[s] * g_j + 2048) >> 12                    the contribution of row j (g_j: its Q12 gain, negative = 0, none = 4096)
//     e_j      = sum_s c_j[s]^2                                  64 bits, exact
//     sel      = all members, or the max_speakers first ones in the order (larger e_j, then smaller row index)
//     S[s]     = sum_{j in sel} c_j[s]                           32 bits, exact (the host refuses calls that could overflow it)
//     out_i[s] = sat16(S[s] - (i in sel ? c_i[s] : 0))
//
// per packet, stateless.  Everything is integer arithmetic with a total selection order, so the output is a pure function of the inputs.
// Five short launches, none of which waits for another workgroup:
//
//     1. clear    the room counters and the call's verdict word
//     2. check    one lane per row: a room id outside [-1, n_rooms) sets the verdict (every later kernel then leaves before it touches
//                 anything, solo_stream_ctl.h); the others are counted per room
//     3. scan     ONE workgroup: a run of rooms per lane, wg_scan_incl over the lanes' sums -> every room's first slot in the member
//                 list (CSR), and the call's counts
//     4. scatter  one lane per row: the row index into its room's list.  The order inside a list is whatever the atomics give; the sums
//                 are integer and the selection order is total, so the result does not depend on it
//     5. mix      ONE wavefront per (room, packet), which walks the room's members (sx_mix_unit)
//
// The mix is memory bound (2 x L bytes in and out per row and packet).  Every PCM access is 16 bytes per lane (8 samples; a row is
// L / 8 = 40, 80 or 160 such chunks, lane l of the wave owns chunks l, l + 64, l + 128), S lives in registers, and rows are requested as
// few times as the data flow allows:
//   * every member mixed (max_speakers <= 0 or >= the room): pass 1 reads each row (energy, S), pass 2 reads it again for S - c_i.  The
//     first SX_MIX_CACHE_CHUNKS / (L / 8) members of the list (8 at L = 640) are kept in LDS by pass 1, so a small room is read ONCE;
//   * a selection (max_speakers < the room): pass 1 reads each row for its energy; max_speakers rounds of a wave-wide arg-best over the
//     energies (each round: the best key that comes after the previous pick) choose sel; the chosen rows are read a second time for S and
//     kept in LDS for their own S - c_i (those beyond the cache, possible from max_speakers 9 at L = 640, are read a third time -- at
//     most 64 rows of the room); every other member hears sat16(S), which is computed once and stored without reading anything.
// Every output row is written once, no atomics touch PCM, and `clipped` is one atomic per workgroup.
//
// Everything outside the kernels compiles for the host as well (tests/test_mix_model.py builds sx_mix_host: the passes run through the
// very functions of the kernels, with the 1-lane forms of solo_wave.h, and are compared with an independent model).
#pragma once
#include "solo_wave.h"
#include "solo_stream_ctl.h"
#include "../../include/solo_mi355x.h"

#define SX_MIX_MAX_SPEAKERS 64
#define SX_MIX_MAX_L 1280                                   // samples of the longest packet (40 ms at 32 kHz)
#define SX_MIX_CACHE_CHUNKS 640                             // 16-byte chunks of PCM a (room, packet) keeps in LDS: 10 KB, 8 rows of 640 samples
#define SX_MIX_ITERS ((SX_MIX_MAX_L / 8 + SX_NLANES - 1) / SX_NLANES)       // chunks per lane and row: 3 (160 in the 1-lane host form)
#define SX_MIX_MAX_ALL_ROWS 8191                            // rows of a call that may mix every member: 8191 x 2^18 < 2^31

typedef solo_mix_count_t SxMixCount;
static_assert(sizeof(SxMixCount) == 16, "solo_mix_count_t layout");

struct alignas(16) SxMixX8 { i16 s[8]; };                   // what one lane loads and stores

struct SxMixArgs {
    const i16* pcm_in; const i16* gain; i16* pcm_out;
    i64* energy; u8* mixed;                                 // [n][n_packets]: the caller's, or the handle's scratch (the selection reads both back)
    const i32* counts; const i32* starts; const i32* members;      // the room plan: members[starts[r] .. + counts[r]) are the rows of room r
    int n_packets, L, max_speakers;
};

SX_HD i32 sx_mix_gain(const i16* gain, int row) {
    if (!gain) return 4096;
    const i32 g = gain[row];
    return g < 0 ? 0 : g;
}
SX_HD i32 sx_mix_contrib(i32 x, i32 g) { return (x * g + 2048) >> 12; }
SX_HD i16 sx_mix_sat(i32 v, i32* clipped) {
    const i32 s = v > 32767 ? 32767 : (v < -32768 ? -32768 : v);
    *clipped += (s != v);
    return (i16)s;
}
// the selection order: does (energy ea, row ia) come before (eb, ib)?
SX_HD bool sx_mix_before(i64 ea, i32 ia, i64 eb, i32 ib) { return ea > eb || (ea == eb && ia < ib); }
// the first key of the wave in that order, in every lane
SX_HD void wv_mix_best(i64* e, i32* idx) {
#if defined(__HIP_DEVICE_COMPILE__) && SX_NLANES == 64
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const i64 te = __shfl_xor(*e, o, 64);
        const i32 ti = __shfl_xor(*idx, o, 64);
        if (sx_mix_before(te, ti, *e, *idx)) { *e = te; *idx = ti; }
    }
#else
    (void)e; (void)idx;
#endif
}
// lane t's value (t wave-uniform)
SX_HD i32 sx_mix_lane(i32 v, int t) {
#if defined(__HIP_DEVICE_COMPILE__) && SX_NLANES == 64
    return __builtin_amdgcn_readlane(v, t);
#else
    (void)t;
    return v;
#endif
}

// this lane's chunks of a row
SX_HD void sx_mix_load(const SxMixX8* row, int CH, SxMixX8 (&x)[SX_MIX_ITERS]) {
#pragma unroll
    for (int k = 0; k < SX_MIX_ITERS; k++) {
        const int ch = k * SX_NLANES + SX_LANE;
        if (ch < CH) x[k] = row[ch];
    }
}
// a row's contribution: its energy (the wave's, in every lane), and -- with `add` -- c_j into S
SX_HD i64 sx_mix_first(const SxMixX8 (&x)[SX_MIX_ITERS], int CH, i32 g, bool add, i32 (&S)[SX_MIX_ITERS][8]) {
    i64 e = 0;
#pragma unroll
    for (int k = 0; k < SX_MIX_ITERS; k++) {
        const int ch = k * SX_NLANES + SX_LANE;
        if (ch < CH) {
#pragma unroll
            for (int s = 0; s < 8; s++) {
                const i32 c = sx_mix_contrib(x[k].s[s], g);
                e += (i64)c * (i64)c;
                if (add) S[k][s] += c;
            }
        }
    }
    return wv_sum64(e);
}
// out = sat16(S - c) for a mixed row (minus = true), sat16(S) otherwise; -> this lane's saturated samples
SX_HD i32 sx_mix_second(const SxMixX8 (&x)[SX_MIX_ITERS], int CH, i32 g, bool minus, const i32 (&S)[SX_MIX_ITERS][8], SxMixX8* out) {
    i32 clipped = 0;
#pragma unroll
    for (int k = 0; k < SX_MIX_ITERS; k++) {
        const int ch = k * SX_NLANES + SX_LANE;
        if (ch < CH) {
            SxMixX8 o;
#pragma unroll
            for (int s = 0; s < 8; s++) o.s[s] = sx_mix_sat(S[k][s] - (minus ? sx_mix_contrib(x[k].s[s], g) : 0), &clipped);
            out[ch] = o;
        }
    }
    return clipped;
}
SX_HD void sx_mix_cache_put(SxMixX8* slot, int CH, const SxMixX8 (&x)[SX_MIX_ITERS]) {
#pragma unroll
    for (int k = 0; k < SX_MIX_ITERS; k++) {
        const int ch = k * SX_NLANES + SX_LANE;
        if (ch < CH) slot[ch] = x[k];
    }
}

// The selection, of solo_vad_select (solo_vad.h) as well: K rounds of a wave-wide arg-best over the keys (key(row), row) of a room's m
// members; round k picks the first key that comes after pick k - 1 and hands it to pick(k, row, key).  A key below -1 is no candidate.
// A round that finds none ends the selection, so that no caller indexes a row by the sentinel (with K < m and no key negative there
// always is one: solo_mix, solo_mix_shared) -> the picks made
template <typename Key, typename Pick>
SX_HD int sx_mix_select(const i32* mem, int m, int K, Key key, Pick pick) {
    i64 pe = 0;
    i32 pi = 0;
    for (int k = 0; k < K; k++) {
        i64 be = -1;                                        // (any candidate beats this)
        i32 bi = 0x7FFFFFFF;
        for (int j = SX_LANE; j < m; j += SX_NLANES) {
            const i32 row = mem[j];
            const i64 e = key(row);
            if ((k == 0 || sx_mix_before(pe, pi, e, row)) && sx_mix_before(e, row, be, bi)) { be = e; bi = row; }
        }
        wv_mix_best(&be, &bi);
        if (bi == 0x7FFFFFFF) return k;
        pick(k, bi, be);
        pe = be; pi = bi;
    }
    return K;
}
// what everybody who was not picked hears: o = sat16(S), this lane's chunks, computed once -> this lane's saturated samples of it
SX_HD i32 sx_mix_sat_tile(const i32 (&S)[SX_MIX_ITERS][8], int CH, SxMixX8 (&o)[SX_MIX_ITERS]) {
    i32 clip_s = 0;
#pragma unroll
    for (int k = 0; k < SX_MIX_ITERS; k++)
#pragma unroll
        for (int s = 0; s < 8; s++) o[k].s[s] = (k * SX_NLANES + SX_LANE < CH) ? sx_mix_sat(S[k][s], &clip_s) : (i16)0;
    return clip_s;
}

// One (room, packet): what one wavefront does.  cache: SX_MIX_CACHE_CHUNKS chunks, sel: SX_MIX_MAX_SPEAKERS words (LDS on the device).
// -> the saturated output samples of the unit (the wave's total, in every lane)
SX_HD i64 sx_mix_unit(const SxMixArgs& a, int room, int p, SxMixX8* cache, i32* sel) {
    const int m = SX_UNI(a.counts[room]);
    if (m <= 0) return 0;
    const i32* mem = a.members + SX_UNI(a.starts[room]);
    const int CH = a.L >> 3, P = a.n_packets;
    int K = (a.max_speakers <= 0 || a.max_speakers >= m) ? m : a.max_speakers;
    const bool choose = K < m;
    const int cache_rows = SX_MIX_CACHE_CHUNKS / CH;
    const size_t row_chunks = (size_t)P * (size_t)CH;       // chunks between rows
    const SxMixX8* in_p = (const SxMixX8*)a.pcm_in + (size_t)p * (size_t)CH;
    SxMixX8* out_p = (SxMixX8*)a.pcm_out + (size_t)p * (size_t)CH;
    i32 S[SX_MIX_ITERS][8];
#pragma unroll
    for (int k = 0; k < SX_MIX_ITERS; k++)
#pragma unroll
        for (int s = 0; s < 8; s++) S[k][s] = 0;
    i64 clipped = 0;

    // pass 1: every member's energy; without a selection also S, and the head of the list into the cache.  The lanes fetch 64 row
    // indices at a time; two rows are in flight per step.
    for (int j0 = 0; j0 < m; j0 += SX_NLANES) {
        const int jl = j0 + SX_LANE;
        const i32 row_l = jl < m ? mem[jl] : 0;
        if (jl < m) a.mixed[(size_t)row_l * P + p] = choose ? 0 : 1;
        const int nb = sx_min(SX_NLANES, m - j0);
        for (int t = 0; t < nb; t += 2) {
            const int ra = sx_mix_lane(row_l, t), rb = t + 1 < nb ? sx_mix_lane(row_l, t + 1) : -1;
            SxMixX8 xa[SX_MIX_ITERS], xb[SX_MIX_ITERS];
            sx_mix_load(in_p + (size_t)ra * row_chunks, CH, xa);
            if (rb >= 0) sx_mix_load(in_p + (size_t)rb * row_chunks, CH, xb);
            const i64 ea = sx_mix_first(xa, CH, sx_mix_gain(a.gain, ra), !choose, S);
            if (SX_LANE == 0) a.energy[(size_t)ra * P + p] = ea;
            if (!choose && j0 + t < cache_rows) sx_mix_cache_put(cache + (j0 + t) * CH, CH, xa);
            if (rb >= 0) {
                const i64 eb = sx_mix_first(xb, CH, sx_mix_gain(a.gain, rb), !choose, S);
                if (SX_LANE == 0) a.energy[(size_t)rb * P + p] = eb;
                if (!choose && j0 + t + 1 < cache_rows) sx_mix_cache_put(cache + (j0 + t + 1) * CH, CH, xb);
            }
        }
    }
    wv_sync();

    if (!choose) {
        // pass 2: S - c_i for every member, from the cache or from memory
        for (int j0 = 0; j0 < m; j0 += SX_NLANES) {
            const int jl = j0 + SX_LANE;
            const i32 row_l = jl < m ? mem[jl] : 0;
            const int nb = sx_min(SX_NLANES, m - j0);
            for (int t = 0; t < nb; t += 2) {
                const int ja = j0 + t;
                const int ra = sx_mix_lane(row_l, t), rb = t + 1 < nb ? sx_mix_lane(row_l, t + 1) : -1;
                SxMixX8 xa[SX_MIX_ITERS], xb[SX_MIX_ITERS];
                if (ja < cache_rows) sx_mix_load(cache + ja * CH, CH, xa);
                else sx_mix_load(in_p + (size_t)ra * row_chunks, CH, xa);
                if (rb >= 0 && ja + 1 < cache_rows) sx_mix_load(cache + (ja + 1) * CH, CH, xb);
                else if (rb >= 0) sx_mix_load(in_p + (size_t)rb * row_chunks, CH, xb);
                clipped += sx_mix_second(xa, CH, sx_mix_gain(a.gain, ra), true, S, out_p + (size_t)ra * row_chunks);
                if (rb >= 0) clipped += sx_mix_second(xb, CH, sx_mix_gain(a.gain, rb), true, S, out_p + (size_t)rb * row_chunks);
            }
        }
        return wv_sum64(clipped);
    }

    K = sx_mix_select(mem, m, K, [&](i32 row) { return a.energy[(size_t)row * P + p]; },
                      [&](int k, i32 row, i64) { if (SX_LANE == 0) { sel[k] = row; a.mixed[(size_t)row * P + p] = 1; } });
    wv_sync();
    // S over the chosen rows (their second read), which stay in the cache for their own output
    for (int k = 0; k < K; k++) {
        const int row = SX_UNI(sel[k]);
        SxMixX8 x[SX_MIX_ITERS];
        sx_mix_load(in_p + (size_t)row * row_chunks, CH, x);
        (void)sx_mix_first(x, CH, sx_mix_gain(a.gain, row), true, S);
        if (k < cache_rows) sx_mix_cache_put(cache + k * CH, CH, x);
    }
    wv_sync();
    for (int k = 0; k < K; k++) {
        const int row = SX_UNI(sel[k]);
        SxMixX8 x[SX_MIX_ITERS];
        if (k < cache_rows) sx_mix_load(cache + k * CH, CH, x);
        else sx_mix_load(in_p + (size_t)row * row_chunks, CH, x);
        clipped += sx_mix_second(x, CH, sx_mix_gain(a.gain, row), true, S, out_p + (size_t)row * row_chunks);
    }
    // everybody else hears sat16(S): computed once, stored per row, nothing read but the flags
    SxMixX8 o[SX_MIX_ITERS];
    const i32 clip_s = sx_mix_sat_tile(S, CH, o);
    for (int j0 = 0; j0 < m; j0 += SX_NLANES) {
        const int jl = j0 + SX_LANE;
        const i32 row_l = jl < m ? mem[jl] : 0;
        const i32 flag_l = jl < m ? (i32)a.mixed[(size_t)row_l * P + p] : 1;
        const int nb = sx_min(SX_NLANES, m - j0);
        for (int t = 0; t < nb; t++) {
            if (sx_mix_lane(flag_l, t)) continue;
            sx_mix_cache_put(out_p + (size_t)sx_mix_lane(row_l, t) * row_chunks, CH, o);
            clipped += clip_s;
        }
    }
    return wv_sum64(clipped);
}

// The room plan, of solo_mix, solo_mix_shared, solo_mix_selected and solo_vad_select alike: members[starts[r] .. + counts[r]) are the rows
// of room r; cursor[] is what the scatter counts up.  Four arrays of n words (n_rooms <= n) carved out of scratch at `at`; what a stage
// keeps behind them starts at sx_room_plan_end.
struct SxRoomPlan { i32* counts; i32* starts; i32* cursor; i32* members; };
static inline size_t sx_room_plan_bytes(int n) { return 4 * (size_t)n * sizeof(i32); }
static inline SxRoomPlan sx_room_plan(void* at, int n) {
    SxRoomPlan rp;
    rp.counts = (i32*)at; rp.starts = rp.counts + n; rp.cursor = rp.starts + n; rp.members = rp.cursor + n;
    return rp;
}
static inline i32* sx_room_plan_end(const SxRoomPlan& rp, int n) { return rp.members + n; }

// bytes of device scratch a call needs (n_rooms <= n): energy [n][P] | the room plan | mixed [n][P]
static inline size_t solo_mix_scratch_bytes(int n, int n_packets) {
    const size_t np = (size_t)n * (size_t)n_packets;
    return np * sizeof(i64) + sx_room_plan_bytes(n) + np;
}
struct SxMixPlan { i64* energy; SxRoomPlan rooms; u8* mixed; };
static inline SxMixPlan solo_mix_plan(void* scratch, int n, int n_packets) {
    SxMixPlan pl;
    pl.energy = (i64*)scratch;
    pl.rooms = sx_room_plan(pl.energy + (size_t)n * (size_t)n_packets, n);
    pl.mixed = (u8*)sx_room_plan_end(pl.rooms, n);
    return pl;
}

#if defined(__HIPCC__)
__global__ void __launch_bounds__(256) solo_mix_clear_kernel(i32* __restrict__ counts, int n_rooms, u32* verdict) {
    const int r = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (r < n_rooms) counts[r] = 0;
    if (r == 0) *verdict = 0;
}
__global__ void __launch_bounds__(256) solo_mix_check_kernel(const i32* __restrict__ room, int n, int n_rooms, i32* counts, u32* verdict) {
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= n) return;
    const i32 r = room[i];
    if (r < -1 || r >= n_rooms) atomicOr(verdict, 1u);
    else if (r >= 0) atomicAdd(&counts[r], 1);
}
// one workgroup: lane t owns the rooms [t * per, (t + 1) * per)
__global__ void __launch_bounds__(256) solo_mix_scan_kernel(const i32* __restrict__ counts, int n_rooms, i32* __restrict__ starts, i32* __restrict__ cursor,
                                                            SxMixCount* count, const i32* room, const u32* verdict) {
    __shared__ i32 part[2][4];                              // rows, rooms
    if (sx_map_refused(room, verdict)) {
        if (threadIdx.x == 0 && count) count->rows = -1;
        return;
    }
    const int tid = (int)threadIdx.x;
    const int per = (n_rooms + 255) / 256;
    const int r0 = sx_min(tid * per, n_rooms), r1 = sx_min(r0 + per, n_rooms);
    i32 rows = 0, rooms = 0;
    for (int r = r0; r < r1; r++) { const i32 c = counts[r]; rows += c; rooms += c > 0; }
    i32 incl[2] = {rows, rooms};
    wg_scan_incl(incl, part);
    i32 base = incl[0] - rows;
    for (int r = r0; r < r1; r++) { starts[r] = base; cursor[r] = base; base += counts[r]; }
    if (tid == 0 && count) {
        SxMixCount c;
        c.rows = wg_total(part[0]); c.rooms = wg_total(part[1]);
        c.clipped = 0;                                      // (the mix adds what each workgroup saturated)
        *count = c;
    }
}
__global__ void __launch_bounds__(256) solo_mix_scatter_kernel(const i32* __restrict__ room, int n, i32* cursor, i32* __restrict__ members, const u32* verdict) {
    if (sx_map_refused(room, verdict)) return;
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= n) return;
    const i32 r = room[i];
    if (r >= 0) members[atomicAdd(&cursor[r], 1)] = i;
}
// one wavefront per (room, packet); the packets of a room are neighbours in the grid as they are in memory
__global__ void __launch_bounds__(64) solo_mix_kernel(const SxMixArgs a, SxMixCount* count, const i32* room_ids, const u32* verdict) {
    __shared__ SxMixX8 cache[SX_MIX_CACHE_CHUNKS];
    __shared__ i32 sel[SX_MIX_MAX_SPEAKERS];
    if (sx_map_refused(room_ids, verdict)) return;
    const int room = (int)blockIdx.x / a.n_packets, p = (int)blockIdx.x - room * a.n_packets;
    const i64 clipped = sx_mix_unit(a, room, p, cache, sel);
    if (threadIdx.x == 0 && count && clipped) atomicAdd((unsigned long long*)&count->clipped, (unsigned long long)clipped);
}

// The room plan's launches.  Its second half, scan and scatter over counts that a check has filled: solo_mix_shared and solo_mix_selected
// come here behind a clear and a check of their own (count NULL: their compaction counts)
static inline void sx_room_plan_finish(const SxRoomPlan& rp, const i32* room, int n, int n_rooms, SxMixCount* count, const u32* verdict, hipStream_t s) {
    hipLaunchKernelGGL(solo_mix_scan_kernel, dim3(1), dim3(256), 0, s, rp.counts, n_rooms, rp.starts, rp.cursor, count, room, verdict);
    hipLaunchKernelGGL(solo_mix_scatter_kernel, dim3((n + 255) / 256), dim3(256), 0, s, room, n, rp.cursor, rp.members, verdict);
}
// ... and all four: clear, check, scan, scatter.  between(verdict) enqueues what else may set the verdict word, behind the clear that
// zeroes it and ahead of everything that reads it (solo_vad_select: its list check)
template <typename Between>
static inline void sx_room_plan_launch(const SxRoomPlan& rp, const i32* room, int n, int n_rooms, SxMixCount* count, u32* verdict, Between between, hipStream_t s) {
    hipLaunchKernelGGL(solo_mix_clear_kernel, dim3((n_rooms + 255) / 256), dim3(256), 0, s, rp.counts, n_rooms, verdict);
    between(verdict);
    hipLaunchKernelGGL(solo_mix_check_kernel, dim3((n + 255) / 256), dim3(256), 0, s, room, n, n_rooms, rp.counts, verdict);
    sx_room_plan_finish(rp, room, n, n_rooms, count, verdict, s);
}

// (scratch: solo_mix_scratch_bytes(n, n_packets) bytes, 16-byte aligned; a.energy / a.mixed NULL = the scratch's)
static inline hipError_t solo_mix_launch(SxMixArgs a, const i32* room, int n, int n_rooms, void* scratch, SxMixCount* count, u32* verdict, hipStream_t s) {
    const SxMixPlan pl = solo_mix_plan(scratch, n, a.n_packets);
    if (!a.energy) a.energy = pl.energy;
    if (!a.mixed) a.mixed = pl.mixed;
    a.counts = pl.rooms.counts; a.starts = pl.rooms.starts; a.members = pl.rooms.members;
    sx_room_plan_launch(pl.rooms, room, n, n_rooms, count, verdict, [](u32*) {}, s);
    hipLaunchKernelGGL(solo_mix_kernel, dim3((unsigned)(n_rooms * a.n_packets)), dim3(64), 0, s, a, count, room, verdict);
    return hipGetLastError();
}
#else
// Host form of the room plan's launches (tests), over counts that start at zero and room ids that are all inside [-1, n_rooms): the member
// lists filled from the LAST row down (the device's order is whatever its atomics give; any order will do) -> rows in rooms, rooms with members
static inline void sx_room_plan_host(const SxRoomPlan& rp, const i32* room, int n, int n_rooms, i32* rows, i32* rooms) {
    *rows = 0; *rooms = 0;
    for (int i = 0; i < n; i++) if (room[i] >= 0) rp.counts[room[i]]++;
    for (int r = 0; r < n_rooms; r++) { rp.starts[r] = rp.cursor[r] = *rows; *rows += rp.counts[r]; *rooms += rp.counts[r] > 0; }
    for (int i = n - 1; i >= 0; i--) if (room[i] >= 0) rp.members[rp.cursor[room[i]]++] = i;
}
// Host form of the launches (tests): the same plan, then every (room, packet) through sx_mix_unit.
// -> false: a room id is outside [-1, n_rooms), nothing but count->rows = -1 is written
static inline bool sx_mix_host(SxMixArgs a, const i32* room, int n, int n_rooms, SxMixCount* count) {
    for (int i = 0; i < n; i++)
        if (room[i] < -1 || room[i] >= n_rooms) {
            if (count) count->rows = -1;
            return false;
        }
    const size_t np = (size_t)n * (size_t)a.n_packets;
    const int cap = sx_max(n, n_rooms);
    i32* words = new i32[4 * (size_t)cap]();
    const SxRoomPlan rp = sx_room_plan(words, cap);
    i64* energy = a.energy ? NULL : new i64[np];
    u8* mixed = a.mixed ? NULL : new u8[np];
    SxMixX8* cache = new SxMixX8[SX_MIX_CACHE_CHUNKS];
    i32 sel[SX_MIX_MAX_SPEAKERS];
    SxMixCount c; c.rows = 0; c.rooms = 0; c.clipped = 0;
    sx_room_plan_host(rp, room, n, n_rooms, &c.rows, &c.rooms);
    if (!a.energy) a.energy = energy;
    if (!a.mixed) a.mixed = mixed;
    a.counts = rp.counts; a.starts = rp.starts; a.members = rp.members;
    for (int r = 0; r < n_rooms; r++)
        for (int p = 0; p < a.n_packets; p++) c.clipped += sx_mix_unit(a, r, p, cache, sel);
    if (count) *count = c;
    delete[] words; delete[] energy; delete[] mixed; delete[] cache;
    return true;
}
#endif

// solo_mix_shared.h -- the mixing bridge with shared listener mixes (solo_mix_shared, include/solo_mi355x.h).  With max_speakers = k every
// member of a room that is not among the selected speakers hears the same samples, sat16(S) (solo_mix.h): this form writes that row ONCE
// per room and a personal row only for the speakers of the call, so that the encoder behind it runs once per room and once per speaker
// instead of once per listener.  c_j, e_j, sel and S are those of solo_mix -- the very functions, the same total order.
//
//     speaker of the call   a row in a room that is in sel in at least one packet of the call, or whose d_keep is non-zero
//     shared room           a room with at least one member that is not a speaker of the call
//     pcm_spk[k][p]         sat16(S_p - (i in sel_p ? c_i : 0)) of the k-th speaker i in increasing row order
//     pcm_room[j][p]        sat16(S_p) of the j-th shared room in increasing room order
//     source[i]             k for a speaker, n + j for another member of the j-th shared room, -1 for a row in no room
//
// Ten short launches, none of which waits for another workgroup:
//
//     1. clear    the room counters and the call's verdict word
//     2. check    one lane per row: a room id outside [-1, n_rooms) or a d_slots that does not grow strictly from a non-negative start sets
//                 the verdict (every later kernel then leaves before it touches anything); members are counted per room, spk[i] = d_keep[i]
//     3. scan, 4. scatter    the room plan of solo_mix (its kernels, sx_room_plan_finish): members[starts[r] .. + counts[r]) are the rows of room r
//     5. energy   ONE wavefront per (row, packet): e_j.  The work is spread over the rows, so one room of thousands costs what thousands of
//                 small rooms cost; no LDS, so nothing but registers bounds the waves per SIMD
//     6. select   one wavefront per (room, packet): max_speakers rounds of a wave-wide arg-best over the energies (solo_mix's); the picks go
//                 to a list in scratch, d_mixed and spk[] are set
//     7. tally    one lane per row: the members of every room that are not speakers
//     8. compact  ONE workgroup: wg_scan_incl over runs of rows (speakers) and of rooms (shared rooms) -> the two lists, source[] of the
//                 speakers, every room's index, the call's counts
//     9. source   one lane per row: source[] of everybody else
//    10. write    one wavefront per (room, packet): S over the picks (at most 64 rows), S - c_i for each of them, sat16(S) once for the
//                 room's row and for every speaker that was not picked in this packet
//
// Every PCM access is 16 bytes per lane, every output row is written once, no atomics touch PCM, `clipped` is one atomic per workgroup.
// The picks are read twice (for S, then for S - c_i); nothing is kept in LDS -- the second read of at most 64 rows comes from the L2.
//
// Everything outside the kernels compiles for the host as well (tests/test_shared_mix_model.py builds sx_mixsh_host: the passes run
// through the very functions of the kernels, with the 1-lane forms of solo_wave.h, and are compared with an independent model).
#pragma once
#include "solo_mix.h"

typedef solo_mix_shared_count_t SxMixShCount;
static_assert(sizeof(SxMixShCount) == 24, "solo_mix_shared_count_t layout");

struct SxMixShArgs {
    const i16* pcm_in; const i16* gain; const i32* room; const u8* keep; const i32* slots;
    i16* pcm_spk; i32* spk_list; i32* spk_rows; i16* pcm_room; i32* room_list; i32* source;
    i64* energy; u8* mixed;                                 // [n][n_packets]: the caller's, or the handle's scratch
    i32* counts; i32* starts; i32* cursor; i32* members;    // the room plan
    i32* spk;                                               // [n]: 1 = a speaker of the call
    i32* nonspk;                                            // [n_rooms]: members that are not
    i32* room_idx;                                          // [n_rooms]: the room's index among the shared ones, or -1
    i32* sel;                                               // [n][n_packets] words: the picks of (room r, packet p) start at starts[r] * P + p * K_r
    int n, n_rooms, n_packets, L, max_speakers;
};

// What the host refuses (solo_api.hip and the host form both ask here).  L: samples per packet.
static inline bool sx_mixsh_args_ok(const void* pcm_in, long long n, long long n_packets, int L, const void* room, long long n_rooms, int max_speakers,
                                    const void* pcm_spk, const void* spk_list, const void* pcm_room, const void* room_list, const void* source,
                                    const void* count) {
    if (!pcm_in || !room || !pcm_spk || !spk_list || !pcm_room || !room_list || !source || !count) return false;
    if (n <= 0 || n_packets <= 0 || n_rooms <= 0 || n_rooms > n || n * n_packets >= (1LL << 31)) return false;
    if (max_speakers < 1 || max_speakers > SX_MIX_MAX_SPEAKERS) return false;
    if (L <= 0 || L > SX_MIX_MAX_L || (L & 7)) return false;
    const uintptr_t row = (uintptr_t)n_packets * (uintptr_t)L * sizeof(i16);
    const uintptr_t lo[3] = {(uintptr_t)pcm_in, (uintptr_t)pcm_spk, (uintptr_t)pcm_room};
    const uintptr_t len[3] = {(uintptr_t)n * row, (uintptr_t)n * row, (uintptr_t)n_rooms * row};
    for (int k = 0; k < 3; k++) {
        if (lo[k] & 15) return false;
        for (int j = 0; j < k; j++)
            if (lo[k] < lo[j] + len[j] && lo[j] < lo[k] + len[k]) return false;
    }
    return true;
}

SX_HD unsigned long long sx_mixsh_ballot(bool v) {
#if defined(__HIP_DEVICE_COMPILE__) && SX_NLANES == 64
    return __ballot(v);
#else
    return v ? 1ull : 0ull;
#endif
}
// the picks a (room of m members, packet) has, and where its list starts
SX_HD int sx_mixsh_picks(const SxMixShArgs& a, int m) { return sx_min(a.max_speakers, m); }
SX_HD i32* sx_mixsh_sel(const SxMixShArgs& a, int start, int K, int p) { return a.sel + (size_t)start * (size_t)a.n_packets + (size_t)p * (size_t)K; }

// pass 5, one (row, packet): what one wavefront does
SX_HD void sx_mixsh_energy_unit(const SxMixShArgs& a, int row, int p) {
    if (SX_UNI(a.room[row]) < 0) return;
    const int CH = a.L >> 3;
    const size_t pk = (size_t)row * (size_t)a.n_packets + (size_t)p;
    SxMixX8 x[SX_MIX_ITERS];
    i32 S[SX_MIX_ITERS][8] = {};                            // (not added to)
    sx_mix_load((const SxMixX8*)a.pcm_in + pk * (size_t)CH, CH, x);
    const i64 e = sx_mix_first(x, CH, sx_mix_gain(a.gain, row), false, S);
    if (SX_LANE == 0) a.energy[pk] = e;
}

// pass 6, one (room, packet): the selection of solo_mix (sx_mix_unit) over energies that are already there
SX_HD void sx_mixsh_select_unit(const SxMixShArgs& a, int room, int p) {
    const int m = SX_UNI(a.counts[room]);
    if (m <= 0) return;
    const int start = SX_UNI(a.starts[room]), P = a.n_packets;
    const i32* mem = a.members + start;
    const int K = sx_mixsh_picks(a, m);
    i32* sel = sx_mixsh_sel(a, start, K, p);
    const bool choose = K < m;
    for (int j = SX_LANE; j < m; j += SX_NLANES) {
        const i32 row = mem[j];
        a.mixed[(size_t)row * P + p] = choose ? 0 : 1;
        if (!choose) { sel[j] = row; a.spk[row] = 1; }      // (m <= 64: everybody is picked, in list order)
    }
    if (!choose) return;
    wv_sync();
    (void)sx_mix_select(mem, m, K, [&](i32 row) { return a.energy[(size_t)row * P + p]; },      // (K < m: K picks)
                  [&](int k, i32 row, i64) { if (SX_LANE == 0) { sel[k] = row; a.mixed[(size_t)row * P + p] = 1; a.spk[row] = 1; } });
}

// pass 10, one (room of m > 0 members, packet) whose K picks are sel[0 .. K) and are flagged in a.mixed (solo_mix_selected.h brings a K
// and a list of its own) -> the saturated output samples of the unit (the wave's total, in every lane)
SX_HD i64 sx_mixsh_write_picks(const SxMixShArgs& a, int room, int p, int m, int start, int K, const i32* sel) {
    const int P = a.n_packets, CH = a.L >> 3;
    const i32* mem = a.members + start;
    const size_t row_chunks = (size_t)P * (size_t)CH;       // chunks between rows
    const SxMixX8* in_p = (const SxMixX8*)a.pcm_in + (size_t)p * (size_t)CH;
    SxMixX8* spk_p = (SxMixX8*)a.pcm_spk + (size_t)p * (size_t)CH;
    i32 S[SX_MIX_ITERS][8];
#pragma unroll
    for (int k = 0; k < SX_MIX_ITERS; k++)
#pragma unroll
        for (int s = 0; s < 8; s++) S[k][s] = 0;
    i64 clipped = 0;
    for (int k = 0; k < K; k++) {
        const int row = SX_UNI(sel[k]);
        SxMixX8 x[SX_MIX_ITERS];
        sx_mix_load(in_p + (size_t)row * row_chunks, CH, x);
        (void)sx_mix_first(x, CH, sx_mix_gain(a.gain, row), true, S);
    }
    for (int k = 0; k < K; k++) {                           // the picks' second read
        const int row = SX_UNI(sel[k]);
        const int dst = SX_UNI(a.source[row]);
        SxMixX8 x[SX_MIX_ITERS];
        sx_mix_load(in_p + (size_t)row * row_chunks, CH, x);
        clipped += sx_mix_second(x, CH, sx_mix_gain(a.gain, row), true, S, spk_p + (size_t)dst * row_chunks);
    }
    if (K == m) return wv_sum64(clipped);                   // (everybody was picked: no room row, no other speaker)
    // sat16(S): computed once, stored for the room and for every speaker of the call that was not picked here
    SxMixX8 o[SX_MIX_ITERS];
    const i32 clip_s = sx_mix_sat_tile(S, CH, o);
    const int ri = SX_UNI(a.room_idx[room]);
    if (ri >= 0) {
        sx_mix_cache_put((SxMixX8*)a.pcm_room + ((size_t)ri * (size_t)P + (size_t)p) * (size_t)CH, CH, o);
        clipped += clip_s;
    }
    for (int j0 = 0; j0 < m; j0 += SX_NLANES) {
        const int jl = j0 + SX_LANE;
        const i32 row_l = jl < m ? mem[jl] : 0;
        const bool need_l = jl < m && a.spk[row_l] != 0 && a.mixed[(size_t)row_l * P + p] == 0;
        const i32 dst_l = need_l ? a.source[row_l] : 0;
        unsigned long long todo = sx_mixsh_ballot(need_l);
        while (todo) {
            const int t = __builtin_ctzll(todo);
            todo &= todo - 1;
            sx_mix_cache_put(spk_p + (size_t)sx_mix_lane(dst_l, t) * row_chunks, CH, o);
            clipped += clip_s;
        }
    }
    return wv_sum64(clipped);
}
SX_HD i64 sx_mixsh_write_unit(const SxMixShArgs& a, int room, int p) {
    const int m = SX_UNI(a.counts[room]);
    if (m <= 0) return 0;
    const int start = SX_UNI(a.starts[room]), K = sx_mixsh_picks(a, m);
    return sx_mixsh_write_picks(a, room, p, m, start, K, sx_mixsh_sel(a, start, K, p));
}

// The words per row of a call (n_rooms <= n), of solo_mix_selected as well: the room plan (solo_mix.h) | speaker flags, non-speaker counts,
// room indices, carved out of scratch at `at` -> what lies behind them
static inline size_t sx_mixsh_rows_bytes(int n) { return sx_room_plan_bytes(n) + 3 * (size_t)n * sizeof(i32); }
static inline i32* sx_mixsh_rows(SxMixShArgs& a, void* at) {
    const SxRoomPlan rp = sx_room_plan(at, a.n);
    a.counts = rp.counts; a.starts = rp.starts; a.cursor = rp.cursor; a.members = rp.members;
    a.spk = sx_room_plan_end(rp, a.n); a.nonspk = a.spk + a.n; a.room_idx = a.nonspk + a.n;
    return a.room_idx + a.n;
}
static inline SxRoomPlan sx_mixsh_rooms(const SxMixShArgs& a) {
    SxRoomPlan rp;
    rp.counts = a.counts; rp.starts = a.starts; rp.cursor = a.cursor; rp.members = a.members;
    return rp;
}
// bytes of device scratch a call needs: energy [n][P] | the words per row | the picks [n][P] | mixed [n][P]
static inline size_t solo_mixsh_scratch_bytes(int n, int n_packets) {
    const size_t np = (size_t)n * (size_t)n_packets;
    return np * sizeof(i64) + sx_mixsh_rows_bytes(n) + np * sizeof(i32) + np;
}
// (a.energy / a.mixed NULL = the scratch's)
static inline void solo_mixsh_plan(SxMixShArgs& a, void* scratch) {
    const size_t np = (size_t)a.n * (size_t)a.n_packets;
    i64* energy = (i64*)scratch;
    a.sel = sx_mixsh_rows(a, energy + np);
    u8* mixed = (u8*)(a.sel + np);
    if (!a.energy) a.energy = energy;
    if (!a.mixed) a.mixed = mixed;
}

#if defined(__HIPCC__)
__global__ void __launch_bounds__(256) solo_mixsh_clear_kernel(i32* __restrict__ counts, i32* __restrict__ nonspk, int n_rooms, u32* verdict) {
    const int r = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (r < n_rooms) { counts[r] = 0; nonspk[r] = 0; }
    if (r == 0) *verdict = 0;
}
__global__ void __launch_bounds__(256) solo_mixsh_check_kernel(const SxMixShArgs a, u32* verdict) {
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= a.n) return;
    const i32 r = a.room[i];
    bool bad = r < -1 || r >= a.n_rooms;
    if (a.slots) {
        const i32 s = a.slots[i];
        bad |= s < 0 || (i > 0 && a.slots[i - 1] >= s);
    }
    if (bad) atomicOr(verdict, 1u);
    else if (r >= 0) atomicAdd(&a.counts[r], 1);
    a.spk[i] = (!bad && r >= 0 && a.keep && a.keep[i]) ? 1 : 0;
}
// four (row, packet) units per workgroup, one per wavefront
__global__ void __launch_bounds__(256) solo_mixsh_energy_kernel(const SxMixShArgs a, const u32* verdict) {
    if (sx_map_refused(a.room, verdict)) return;
    const long long u = (long long)blockIdx.x * 4 + (long long)(threadIdx.x >> 6);
    if (u >= (long long)a.n * a.n_packets) return;
    const int row = (int)(u / a.n_packets);
    sx_mixsh_energy_unit(a, row, (int)(u - (long long)row * a.n_packets));
}
__global__ void __launch_bounds__(64) solo_mixsh_select_kernel(const SxMixShArgs a, const u32* verdict) {
    if (sx_map_refused(a.room, verdict)) return;
    const int room = (int)blockIdx.x / a.n_packets;
    sx_mixsh_select_unit(a, room, (int)blockIdx.x - room * a.n_packets);
}
__global__ void __launch_bounds__(256) solo_mixsh_tally_kernel(const SxMixShArgs a, const u32* verdict) {
    if (sx_map_refused(a.room, verdict)) return;
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= a.n) return;
    const i32 r = a.room[i];
    if (r >= 0 && !a.spk[i]) atomicAdd(&a.nonspk[r], 1);
}
// one workgroup of 256: lane t owns the rows [t * per, (t + 1) * per) and the rooms [t * per_r, (t + 1) * per_r).  -> false, in every lane,
// when the call was refused (solo_mix_selected.h adds counts of its own behind it)
__device__ __forceinline__ bool sx_mixsh_compact_group(const SxMixShArgs& a, SxMixShCount* count, const u32* verdict) {
    __shared__ i32 part[4][4];                              // speakers, shared rooms, rows, rooms
    if (sx_map_refused(a.room, verdict)) {
        if (threadIdx.x == 0) count->rows = -1;
        return false;
    }
    const int tid = (int)threadIdx.x;
    const int per = (a.n + 255) / 256, per_r = (a.n_rooms + 255) / 256;
    const int i0 = sx_min(tid * per, a.n), i1 = sx_min(i0 + per, a.n);
    const int r0 = sx_min(tid * per_r, a.n_rooms), r1 = sx_min(r0 + per_r, a.n_rooms);
    i32 spk = 0, shared = 0, rows = 0, rooms = 0;
    for (int i = i0; i < i1; i++) spk += a.spk[i] != 0;
    for (int r = r0; r < r1; r++) { const i32 c = a.counts[r]; rows += c; rooms += c > 0; shared += a.nonspk[r] > 0; }
    i32 incl[4] = {spk, shared, rows, rooms};
    wg_scan_incl(incl, part);
    i32 k = incl[0] - spk, j = incl[1] - shared;
    for (int i = i0; i < i1; i++)
        if (a.spk[i]) {
            a.source[i] = k;
            a.spk_list[k] = a.slots ? a.slots[i] : i;
            if (a.spk_rows) a.spk_rows[k] = i;
            k++;
        }
    for (int r = r0; r < r1; r++) {
        const bool sh = a.nonspk[r] > 0;
        a.room_idx[r] = sh ? j : -1;
        if (sh) a.room_list[j++] = r;
    }
    if (tid == 0) {
        SxMixShCount c;
        c.rows = wg_total(part[2]); c.rooms = wg_total(part[3]); c.speakers = wg_total(part[0]); c.shared = wg_total(part[1]);
        c.clipped = 0;                                      // (the write pass adds what each workgroup saturated)
        *count = c;
    }
    return true;
}
__global__ void __launch_bounds__(256) solo_mixsh_compact_kernel(const SxMixShArgs a, SxMixShCount* count, const u32* verdict) {
    (void)sx_mixsh_compact_group(a, count, verdict);
}
__global__ void __launch_bounds__(256) solo_mixsh_source_kernel(const SxMixShArgs a, const u32* verdict) {
    if (sx_map_refused(a.room, verdict)) return;
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= a.n) return;
    const i32 r = a.room[i];
    if (r < 0) a.source[i] = -1;
    else if (!a.spk[i]) a.source[i] = a.n + a.room_idx[r];
}
__global__ void __launch_bounds__(64) solo_mixsh_write_kernel(const SxMixShArgs a, SxMixShCount* count, const u32* verdict) {
    if (sx_map_refused(a.room, verdict)) return;
    const int room = (int)blockIdx.x / a.n_packets;
    const i64 clipped = sx_mixsh_write_unit(a, room, (int)blockIdx.x - room * a.n_packets);
    if (threadIdx.x == 0 && clipped) atomicAdd((unsigned long long*)&count->clipped, (unsigned long long)clipped);
}

// (scratch: solo_mixsh_scratch_bytes(n, n_packets) bytes, 16-byte aligned)
static inline hipError_t solo_mixsh_launch(SxMixShArgs a, void* scratch, SxMixShCount* count, u32* verdict, hipStream_t s) {
    solo_mixsh_plan(a, scratch);
    const dim3 rows((a.n + 255) / 256), units((unsigned)(a.n_rooms * a.n_packets));
    const unsigned energy_blocks = (unsigned)(((long long)a.n * a.n_packets + 3) / 4);
    hipLaunchKernelGGL(solo_mixsh_clear_kernel, dim3((a.n_rooms + 255) / 256), dim3(256), 0, s, a.counts, a.nonspk, a.n_rooms, verdict);
    hipLaunchKernelGGL(solo_mixsh_check_kernel, rows, dim3(256), 0, s, a, verdict);
    sx_room_plan_finish(sx_mixsh_rooms(a), a.room, a.n, a.n_rooms, (SxMixCount*)NULL, verdict, s);
    hipLaunchKernelGGL(solo_mixsh_energy_kernel, dim3(energy_blocks), dim3(256), 0, s, a, verdict);
    hipLaunchKernelGGL(solo_mixsh_select_kernel, units, dim3(64), 0, s, a, verdict);
    hipLaunchKernelGGL(solo_mixsh_tally_kernel, rows, dim3(256), 0, s, a, verdict);
    hipLaunchKernelGGL(solo_mixsh_compact_kernel, dim3(1), dim3(256), 0, s, a, count, verdict);
    hipLaunchKernelGGL(solo_mixsh_source_kernel, rows, dim3(256), 0, s, a, verdict);
    hipLaunchKernelGGL(solo_mixsh_write_kernel, units, dim3(64), 0, s, a, count, verdict);
    return hipGetLastError();
}
#else
// Host form of the launches (tests): the same passes in the same order, serially, in three stages that solo_mix_selected.h runs as well.
// the check pass -> false: refused "on the device"
static inline bool sx_mixsh_host_check(const SxMixShArgs& a) {
    for (int i = 0; i < a.n; i++) {
        bool bad = a.room[i] < -1 || a.room[i] >= a.n_rooms;
        if (a.slots) bad |= a.slots[i] < 0 || (i > 0 && a.slots[i - 1] >= a.slots[i]);
        if (bad) return false;
    }
    return true;
}
// the room plan (the scratch starts zeroed): member counts and lists, spk[i] = d_keep[i], the counts rows and rooms
static inline void sx_mixsh_host_rooms(const SxMixShArgs& a, SxMixShCount& c) {
    c.speakers = 0; c.shared = 0; c.clipped = 0;
    for (int i = 0; i < a.n; i++) a.spk[i] = (a.room[i] >= 0 && a.keep && a.keep[i]) ? 1 : 0;
    sx_room_plan_host(sx_mixsh_rooms(a), a.room, a.n, a.n_rooms, &c.rows, &c.rooms);
}
// tally, compact, source: the two lists, source[], every room's index, the counts speakers and shared
static inline void sx_mixsh_host_lists(const SxMixShArgs& a, SxMixShCount& c) {
    const int n = a.n, R = a.n_rooms;
    for (int i = 0; i < n; i++) if (a.room[i] >= 0 && !a.spk[i]) a.nonspk[a.room[i]]++;
    for (int i = 0; i < n; i++)
        if (a.spk[i]) {
            a.source[i] = c.speakers;
            a.spk_list[c.speakers] = a.slots ? a.slots[i] : i;
            if (a.spk_rows) a.spk_rows[c.speakers] = i;
            c.speakers++;
        }
    for (int r = 0; r < R; r++) {
        a.room_idx[r] = a.nonspk[r] > 0 ? c.shared : -1;
        if (a.nonspk[r] > 0) a.room_list[c.shared++] = r;
    }
    for (int i = 0; i < n; i++) {
        if (a.room[i] < 0) a.source[i] = -1;
        else if (!a.spk[i]) a.source[i] = n + a.room_idx[a.room[i]];
    }
}
// -> false: refused "on the device", nothing but count->rows = -1 is written
static inline bool sx_mixsh_host(SxMixShArgs a, SxMixShCount* count) {
    const int n = a.n, R = a.n_rooms, P = a.n_packets;
    if (!sx_mixsh_host_check(a)) { count->rows = -1; return false; }
    const size_t bytes = solo_mixsh_scratch_bytes(n, P);
    i64* scratch = new i64[bytes / sizeof(i64) + 1]();
    solo_mixsh_plan(a, scratch);
    SxMixShCount c;
    sx_mixsh_host_rooms(a, c);
    for (int i = 0; i < n; i++) for (int p = 0; p < P; p++) sx_mixsh_energy_unit(a, i, p);
    for (int r = 0; r < R; r++) for (int p = 0; p < P; p++) sx_mixsh_select_unit(a, r, p);
    sx_mixsh_host_lists(a, c);
    for (int r = 0; r < R; r++) for (int p = 0; p < P; p++) c.clipped += sx_mixsh_write_unit(a, r, p);
    *count = c;
    delete[] scratch;
    return true;
}
#endif

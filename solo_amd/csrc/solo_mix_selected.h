// solo_mix_selected.h -- shared listener mixes from a GIVEN selection (solo_mix_selected, include/solo_mi355x.h): solo_mix_shared without
// its energy and select passes.  The caller says who speaks in every packet (d_sel, what solo_vad_select writes); everything else is
// solo_mix_shared's: c_j, S, the speakers and shared rooms of the call, the two PCM tables, the lists and the source table.
//
//     sel_p(r)              { i in room r : d_sel[i][p] != 0 } -- empty, some, or every member; at most 64 rows
//     speaker of the call   a row in a room that is in sel_p in at least one packet of the call, or whose d_keep is non-zero
//     pcm_spk[k][p]         sat16(S_p - (i in sel_p ? c_i : 0)), S_p = sum over sel_p of c_j
//     pcm_room[j][p]        sat16(S_p); room_nsel[j][p] = |sel_p|: 0 = that packet of the row is digital silence
//
// Nine short launches (ten with d_energy), none of which waits for another workgroup.  Seven are solo_mix_shared's and solo_mix's own
// kernels: clear, check, scan, scatter, (energy,) tally, source.  New:
//
//     gather   one wavefront per (room, packet): the lanes stride over the room's members, each reads its member's d_sel byte; a ballot
//              and a lane prefix count (v_mbcnt) per stride of 64 on top of a wave-uniform running base compact the selected rows into
//              the pick list in scratch (at starts[r] * P + p * m: a room of m members has m words per packet).  The count goes to a word
//              per (room, packet), spk[] is set, and more than 64 picks raise the call's verdict.  Scratch only: the pass runs ahead of
//              everything that writes a caller's buffer, the energy pass included, so that a refusal leaves them all untouched.  The
//              member lists come out of an atomic scatter in any order, and so do the picks; S is an exact integer sum
//     compact  solo_mix_shared's workgroup (sx_mixsh_compact_group), whose lanes then add up the gathered counts of their rooms: the
//              counts `selected` and `silent`.  (Added by the write pass, one atomic per workgroup each, they cost 25 600 atomics on one
//              address at 512 rooms x 50 packets: 0.25 ms of a 0.34 ms call.  Here they are 100 loads per lane and no atomic.)
//     write    solo_mix_shared's sx_mixsh_write_picks with K = the gathered count: K = 0 gives a zero room row and zero rows for kept
//              speakers, K = m no room row.  It writes room_nsel and adds `clipped`, one atomic per workgroup that saturated anything
//
// Every PCM access is 16 bytes per lane; no LDS in gather and write, no scratch memory anywhere.
//
// Everything outside the kernels compiles for the host as well (tests/test_selected_mix_model.py builds sx_mixsel_host: the passes run
// through the very functions of the kernels, with the 1-lane forms of solo_wave.h, and are compared with an independent model).
#pragma once
#include "solo_mix_shared.h"

typedef solo_mix_selected_count_t SxMixSelCount;
static_assert(sizeof(SxMixSelCount) == 32, "solo_mix_selected_count_t layout");

struct SxMixSelArgs {
    SxMixShArgs sh;             // what solo_mix_shared's kernels read: sh.mixed is d_sel (never written here), sh.max_speakers unused
    u8* room_nsel;              // [n_rooms][n_packets], or NULL
    i32* nsel;                  // [n_rooms][n_packets] words of scratch: the picks of (room, packet)
};

// What the host refuses: everything solo_mix_shared refuses (it has no max_speakers), and a NULL d_sel
static inline bool sx_mixsel_args_ok(const void* pcm_in, long long n, long long n_packets, int L, const void* room, long long n_rooms, const void* sel,
                                     const void* pcm_spk, const void* spk_list, const void* pcm_room, const void* room_list, const void* source,
                                     const void* count) {
    return sel && sx_mixsh_args_ok(pcm_in, n, n_packets, L, room, n_rooms, 1, pcm_spk, spk_list, pcm_room, room_list, source, count);
}

// where the picks of (a room of m members at `start`, packet p) are listed
SX_HD i32* sx_mixsel_picks(const SxMixShArgs& a, int start, int m, int p) { return a.sel + (size_t)start * (size_t)a.n_packets + (size_t)p * (size_t)m; }
// the lanes below this one whose bit is set
SX_HD int sx_mixsel_lanes_below(unsigned long long mask) {
#if defined(__HIP_DEVICE_COMPILE__) && SX_NLANES == 64
    return (int)__builtin_amdgcn_mbcnt_hi((u32)(mask >> 32), __builtin_amdgcn_mbcnt_lo((u32)mask, 0u));
#else
    (void)mask;
    return 0;
#endif
}

// the gather pass, one (room, packet) -> the picks (in every lane; above SX_MIX_MAX_SPEAKERS the call is refused)
SX_HD int sx_mixsel_gather_unit(const SxMixSelArgs& a, int room, int p) {
    const int m = SX_UNI(a.sh.counts[room]);
    if (m <= 0) return 0;
    const int start = SX_UNI(a.sh.starts[room]), P = a.sh.n_packets;
    const i32* mem = a.sh.members + start;
    i32* picks = sx_mixsel_picks(a.sh, start, m, p);
    int base = 0;                                           // wave-uniform: the picks of the strides before this one
    for (int j0 = 0; j0 < m; j0 += SX_NLANES) {
        const int jl = j0 + SX_LANE;
        const i32 row = jl < m ? mem[jl] : 0;
        const bool on = jl < m && a.sh.mixed[(size_t)row * P + p] != 0;
        const unsigned long long mask = sx_mixsh_ballot(on);
        if (on) {                                           // (base + lanes below < m: the list cannot overflow whatever d_sel holds)
            picks[base + sx_mixsel_lanes_below(mask)] = row;
            a.sh.spk[row] = 1;
        }
        base += __builtin_popcountll(mask);
    }
    if (SX_LANE == 0) a.nsel[(size_t)room * P + p] = base;
    return base;
}

// the counts of one room over the call's packets, behind the tally pass: its picks, and its packets without any if the room is shared
SX_HD void sx_mixsel_room_counts(const SxMixSelArgs& a, int room, i32* selected, i32* silent) {
    if (a.sh.counts[room] <= 0) return;                     // (no member: the gather pass left its words alone)
    const int P = a.sh.n_packets;
    const bool shared = a.sh.nonspk[room] > 0;
    for (int p = 0; p < P; p++) {
        const i32 k = a.nsel[(size_t)room * P + p];
        *selected += k;
        *silent += (shared && k == 0) ? 1 : 0;
    }
}

// the write pass, one (room, packet) -> the saturated output samples of the unit (the wave's total, in every lane)
SX_HD i64 sx_mixsel_write_unit(const SxMixSelArgs& a, int room, int p) {
    const int m = SX_UNI(a.sh.counts[room]);
    if (m <= 0) return 0;
    const int start = SX_UNI(a.sh.starts[room]), P = a.sh.n_packets;
    const int K = SX_UNI(a.nsel[(size_t)room * P + p]);
    const int ri = SX_UNI(a.sh.room_idx[room]);
    if (ri >= 0 && a.room_nsel && SX_LANE == 0) a.room_nsel[(size_t)ri * P + p] = (u8)K;
    return sx_mixsh_write_picks(a.sh, room, p, m, start, K, sx_mixsel_picks(a.sh, start, m, p));
}

// bytes of device scratch a call needs (n_rooms <= n): solo_mix_shared's words per row | the picks [n][P] | their number per (room,
// packet) [n_rooms][P]
static inline size_t solo_mixsel_scratch_bytes(int n, int n_packets) {
    const size_t np = (size_t)n * (size_t)n_packets;
    return sx_mixsh_rows_bytes(n) + 2 * np * sizeof(i32);
}
static inline void solo_mixsel_plan(SxMixSelArgs& a, void* scratch) {
    a.sh.sel = sx_mixsh_rows(a.sh, scratch);
    a.nsel = a.sh.sel + (size_t)a.sh.n * (size_t)a.sh.n_packets;
}

#if defined(__HIPCC__)
__global__ void __launch_bounds__(64) solo_mixsel_gather_kernel(const SxMixSelArgs a, u32* verdict) {
    if (sx_map_refused(a.sh.room, verdict)) return;
    const int room = (int)blockIdx.x / a.sh.n_packets;
    const int picks = sx_mixsel_gather_unit(a, room, (int)blockIdx.x - room * a.sh.n_packets);
    if (threadIdx.x == 0 && picks > SX_MIX_MAX_SPEAKERS) atomicOr(verdict, 1u);
}
__global__ void __launch_bounds__(256) solo_mixsel_compact_kernel(const SxMixSelArgs a, SxMixSelCount* count, const u32* verdict) {
    __shared__ i32 part[2][4];                              // selected, silent
    if (!sx_mixsh_compact_group(a.sh, (SxMixShCount*)count, verdict)) return;
    const int tid = (int)threadIdx.x, per_r = (a.sh.n_rooms + 255) / 256;
    const int r0 = sx_min(tid * per_r, a.sh.n_rooms), r1 = sx_min(r0 + per_r, a.sh.n_rooms);
    i32 selected = 0, silent = 0;
    for (int r = r0; r < r1; r++) sx_mixsel_room_counts(a, r, &selected, &silent);
    i32 incl[2] = {selected, silent};                       // (only the totals are wanted: the scan's one barrier, where two wg_sum take four)
    wg_scan_incl(incl, part);
    if (tid == 0) { count->selected = wg_total(part[0]); count->silent = wg_total(part[1]); }
}
__global__ void __launch_bounds__(64) solo_mixsel_write_kernel(const SxMixSelArgs a, SxMixSelCount* count, const u32* verdict) {
    if (sx_map_refused(a.sh.room, verdict)) return;
    const int room = (int)blockIdx.x / a.sh.n_packets;
    const i64 clipped = sx_mixsel_write_unit(a, room, (int)blockIdx.x - room * a.sh.n_packets);
    if (threadIdx.x == 0 && clipped) atomicAdd((unsigned long long*)&count->clipped, (unsigned long long)clipped);
}

// (scratch: solo_mixsel_scratch_bytes(n, n_packets) bytes, 16-byte aligned; a.sh.energy NULL: no energy pass)
static inline hipError_t solo_mixsel_launch(SxMixSelArgs a, void* scratch, SxMixSelCount* count, u32* verdict, hipStream_t s) {
    solo_mixsel_plan(a, scratch);
    const SxMixShArgs& h = a.sh;
    const dim3 rows((h.n + 255) / 256), units((unsigned)(h.n_rooms * h.n_packets));
    hipLaunchKernelGGL(solo_mixsh_clear_kernel, dim3((h.n_rooms + 255) / 256), dim3(256), 0, s, h.counts, h.nonspk, h.n_rooms, verdict);
    hipLaunchKernelGGL(solo_mixsh_check_kernel, rows, dim3(256), 0, s, h, verdict);
    sx_room_plan_finish(sx_mixsh_rooms(h), h.room, h.n, h.n_rooms, (SxMixCount*)NULL, verdict, s);
    hipLaunchKernelGGL(solo_mixsel_gather_kernel, units, dim3(64), 0, s, a, verdict);
    if (h.energy) {
        const unsigned energy_blocks = (unsigned)(((long long)h.n * h.n_packets + 3) / 4);
        hipLaunchKernelGGL(solo_mixsh_energy_kernel, dim3(energy_blocks), dim3(256), 0, s, h, verdict);
    }
    hipLaunchKernelGGL(solo_mixsh_tally_kernel, rows, dim3(256), 0, s, h, verdict);
    hipLaunchKernelGGL(solo_mixsel_compact_kernel, dim3(1), dim3(256), 0, s, a, count, verdict);
    hipLaunchKernelGGL(solo_mixsh_source_kernel, rows, dim3(256), 0, s, h, verdict);
    hipLaunchKernelGGL(solo_mixsel_write_kernel, units, dim3(64), 0, s, a, count, verdict);
    return hipGetLastError();
}
#else
// Host form of the launches (tests): the same passes in the same order, serially.  -> false: refused "on the device", nothing but
// count->rows = -1 is written
static inline bool sx_mixsel_host(SxMixSelArgs a, SxMixSelCount* count) {
    const int n = a.sh.n, R = a.sh.n_rooms, P = a.sh.n_packets;
    if (!sx_mixsh_host_check(a.sh)) { count->rows = -1; return false; }
    i32* scratch = new i32[solo_mixsel_scratch_bytes(n, P) / sizeof(i32) + 1]();
    solo_mixsel_plan(a, scratch);
    SxMixShCount c;
    sx_mixsh_host_rooms(a.sh, c);
    bool ok = true;
    for (int r = 0; r < R; r++) for (int p = 0; p < P; p++) ok &= sx_mixsel_gather_unit(a, r, p) <= SX_MIX_MAX_SPEAKERS;
    if (!ok) { count->rows = -1; delete[] scratch; return false; }
    if (a.sh.energy) for (int i = 0; i < n; i++) for (int p = 0; p < P; p++) sx_mixsh_energy_unit(a.sh, i, p);
    sx_mixsh_host_lists(a.sh, c);
    SxMixSelCount out;
    out.selected = 0; out.silent = 0;
    for (int r = 0; r < R; r++) sx_mixsel_room_counts(a, r, &out.selected, &out.silent);
    for (int r = 0; r < R; r++) for (int p = 0; p < P; p++) c.clipped += sx_mixsel_write_unit(a, r, p);
    out.rows = c.rows; out.rooms = c.rooms; out.speakers = c.speakers; out.shared = c.shared; out.clipped = c.clipped;
    *count = out;
    delete[] scratch;
    return true;
}
#endif

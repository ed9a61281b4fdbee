// solo_rate.h -- the sender's feedback loop on the device: a loss-based rate controller with a state record per row (solo_rate_update),
// and its mode as a send mask for solo_send_pack (solo_rate_send_mask); include/solo_mi355x.h states the rule, tests/rate_model.py is
// the same rule in plain Python integers.  What applies the controller's decision to the encoder, solo_batch_update_rates, is a kernel
// of each encoder build (solo_enc_kernels.h: solo_enc_rate_list_kernel) over sx_enc_apply_target (solo_enc_state.h); its call check
// is here.
//
// The controller reads the 32-byte feedback rows that solo_rtcp_parse wrote and writes, per row, the new target (0 where it did not
// change: the input format of solo_batch_update_rates, so only changed streams are touched) and the mode (1: one description per
// packet, alternating).  Integers only, every product in 64 bits, a total rule: the output is a pure function of feedback, parameters
// and state, whatever a state blob held.
//
// The state record of a row is 16 words (SxRateRow): flags, target_bps, last_ehs, min_rtt, idle, over, under, two counters (reports
// used, targets changed), the last fraction_lost and rtt for the host to read, five words that the stage never writes.
//
// The kernels: ONE LANE per row, 256 a workgroup.  A row's step is serial and a few dozen instructions, so there is nothing to spread
// over lanes; the 32-byte feedback row and the 64-byte record are read and written as 16-byte accesses.  The counts go through wg_sum
// (three fields of 10 bits side by side: a workgroup counts at most 256 of each) and one atomic instruction per workgroup (lane k adds
// field k) behind a clear kernel -- a kernel, not a memset node: solo_rtp.h, solo_rtp_clear_kernel says why.  The parameters travel as
// kernel arguments.
//
// Everything outside the kernels compiles for the host as well (tests/rate_host.cpp walks the rows through the very functions of the
// kernels; tests/test_rate_model.py compares them with the independent model).
#pragma once
#include <stddef.h>
#include "solo_enc_state.h"     // sx_enc_apply_target
#include "solo_wave.h"          // wg_sum
#include "solo_stream_ctl.h"    // sx_map_ok
#include "../../include/solo_mi355x.h"

#define SX_RATE_TILE 256        // rows per workgroup = its lanes (wg_sum is for 256)
#define SX_RATE_STATE_WORDS 16
#define SX_RATE_LIVE_WORDS 11   // the words the stage writes; a BYE puts them back to sx_rate_init_word
#define SX_RATE_STARTED 1       // flags: the row has a target
#define SX_RATE_HAS_REPORT 2    // ... has used a report: last_ehs counts
#define SX_RATE_THIN 4          // ... sends one description per packet
#define SX_RATE_MAX_BPS 1000000

// The state record, defined here once; solo_rate_get_state / _set_state move it as it is.
struct SxRateRow {
    i32 flags, target_bps;
    u32 last_ehs;
    i32 min_rtt, idle, over, under;
    u32 n_used, n_changed;      // reports used and targets changed since the reset, mod 2^32
    i32 last_fraction, last_rtt;
    i32 reserved[5];            // never written
};
static_assert(sizeof(SxRateRow) == SOLO_RATE_STATE_BYTES && SOLO_RATE_STATE_BYTES == 4 * SX_RATE_STATE_WORDS, "a row of the state");
static_assert(offsetof(SxRateRow, reserved) == 4 * SX_RATE_LIVE_WORDS, "the live words of a row");
typedef solo_rate_params_t SxRateParams;
typedef solo_rate_count_t SxRateCount;
typedef solo_rate_apply_count_t SxRateApplyCount;
static_assert(sizeof(SxRateParams) == 48 && sizeof(SxRateCount) == 64 && sizeof(SxRateApplyCount) == 16 && sizeof(solo_rtcp_feedback_t) == 32,
              "solo_rate_*, solo_rtcp_feedback_t layout");
#define SX_RATE_COUNT_WORDS 16

// what a row's step did, one bit per field of the count from `started` on: bit k is word k + 1 of solo_rate_count_t
#define SX_RATE_E_STARTED (1 << 0)
#define SX_RATE_E_USED (1 << 1)
#define SX_RATE_E_REPEATED (1 << 2)
#define SX_RATE_E_INCREASED (1 << 3)
#define SX_RATE_E_DECREASED (1 << 4)
#define SX_RATE_E_HELD (1 << 5)
#define SX_RATE_E_DELAYED (1 << 6)
#define SX_RATE_E_STALE (1 << 7)
#define SX_RATE_E_BYE (1 << 8)
#define SX_RATE_E_THIN_ON (1 << 9)
#define SX_RATE_E_THIN_OFF (1 << 10)
#define SX_RATE_E_THIN_ROW (1 << 11)
#define SX_RATE_E_CHANGED (1 << 12)
#define SX_RATE_N_EVENTS 13
static_assert(offsetof(solo_rate_count_t, started) == 4 && offsetof(solo_rate_count_t, used) == 8 && offsetof(solo_rate_count_t, repeated) == 12 &&
              offsetof(solo_rate_count_t, increased) == 16 && offsetof(solo_rate_count_t, decreased) == 20 && offsetof(solo_rate_count_t, held) == 24 &&
              offsetof(solo_rate_count_t, delayed) == 28 && offsetof(solo_rate_count_t, stale) == 32 && offsetof(solo_rate_count_t, bye) == 36 &&
              offsetof(solo_rate_count_t, thin_on) == 40 && offsetof(solo_rate_count_t, thin_off) == 44 && offsetof(solo_rate_count_t, thin_rows) == 48 &&
              offsetof(solo_rate_count_t, changed) == 4 * SX_RATE_N_EVENTS, "event bit k is word k + 1 of solo_rate_count_t");

// word w of the record the create and reset calls leave: no flag, no target, min_rtt = "none yet"
SX_HD i32 sx_rate_init_word(int w) { return w == 3 ? SX_I32_MAX : 0; }

static inline bool sx_rate_params_ok(const SxRateParams* p) {
    if (!p || p->quantum_bps < 1 || p->min_bps < 1 || p->max_bps > SX_RATE_MAX_BPS || p->min_bps > p->max_bps) return false;
    if (p->start_bps < p->min_bps || p->start_bps > p->max_bps) return false;
    if (p->min_bps % p->quantum_bps || p->max_bps % p->quantum_bps || p->start_bps % p->quantum_bps) return false;
    if (p->lo_q8 < 0 || p->lo_q8 > p->hi_q8 || p->hi_q8 > 255 || p->inc_q8 < 0 || p->inc_q8 > 256) return false;
    return p->rtt_guard >= 0 && p->stale_calls >= 0 && p->thin_after >= 0 && p->thin_release >= 0 && p->reserved == 0;
}
// what the host checks of a call before it enqueues anything (solo_api.hip; the host build of the tests asks the same functions)
static inline bool sx_rate_update_call_ok(i32 n_rows, const void* feedback, const SxRateParams* p, const void* target, const void* mode, const void* count) {
    if (n_rows <= 0 || !feedback || !target || !mode || !count || !sx_rate_params_ok(p)) return false;
    return !((uintptr_t)feedback & 15) && !(((uintptr_t)target | (uintptr_t)count) & 3);
}
// ... of solo_batch_update_rates; the handle's facts: its streams, whether it has an encoder
static inline bool sx_rate_apply_call_ok(i32 n_streams, bool have_enc, const void* streams, i32 n, const void* target, const void* count) {
    if (!have_enc || !target || !count || n <= 0 || n > n_streams || (!streams && n != n_streams)) return false;
    return !(((uintptr_t)streams | (uintptr_t)target | (uintptr_t)count) & 3);
}
// ... of solo_rate_send_mask
static inline bool sx_rate_mask_call_ok(const void* mode, i32 n_rows, const void* streams, i32 n, i32 n_packets, const void* seq_base, const void* send) {
    if (!mode || !send || n_rows <= 0 || n <= 0 || n_packets <= 0 || n > n_rows) return false;
    if ((i64)n * (i64)n_packets >= ((i64)1 << 31)) return false;
    return !(((uintptr_t)streams | (uintptr_t)seq_base) & 3);
}

SX_HD i64 sx_rate_clamp64(i64 v, i64 lo, i64 hi) { return v < lo ? lo : (v > hi ? hi : v); }
SX_HD i32 sx_rate_sat_inc(i32 v) { return v < SX_I32_MAX ? v + 1 : v; }

// the live words of a row as the reset calls leave them (sx_rate_init_word)
SX_HD void sx_rate_row_reset(SxRateRow& r) {
    r.flags = 0; r.target_bps = 0; r.last_ehs = 0; r.min_rtt = SX_I32_MAX; r.idle = 0; r.over = 0; r.under = 0;
    r.n_used = 0; r.n_changed = 0; r.last_fraction = 0; r.last_rtt = 0;
}

// One row, one call: the rule of include/solo_mi355x.h, in its order.  seen, fraction_lost, ext_high_seq, rtt: the row of
// solo_rtcp_feedback_t; *target / *mode: what goes to d_target_bps / d_mode.  -> the SX_RATE_E_* bits of what happened
SX_HD i32 sx_rate_step(SxRateRow& r, const SxRateParams& p, i32 seen, i32 fraction_lost, u32 ext_high_seq, i32 rtt, i32* target, i32* mode) {
    i32 ev = 0;
    bool changed = false;
    // 1. not started: the controller's start rate, reported as a change so that the encoder takes it
    if (!(r.flags & SX_RATE_STARTED)) {
        sx_rate_row_reset(r);
        r.flags = SX_RATE_STARTED; r.target_bps = p.start_bps;
        ev |= SX_RATE_E_STARTED;
        changed = true;
    }
    // 2. BYE: back to the reset record
    if (seen & SOLO_RTCP_BYE) {
        sx_rate_row_reset(r);
        *target = 0; *mode = 0;
        return ev | SX_RATE_E_BYE;
    }
    const i64 old = r.target_bps;
    i64 t = old;
    bool thin = (r.flags & SX_RATE_THIN) != 0;
    // 3. is the report used?  (a block that does not advance ext_high_seq is the same interval again; the difference is wrap-safe)
    const bool blocks = (seen & 0xFFFF) > 0;
    const bool used = blocks && (!(r.flags & SX_RATE_HAS_REPORT) || (i32)(ext_high_seq - r.last_ehs) > 0);
    if (blocks && !used) ev |= SX_RATE_E_REPEATED;
    if (!used) {
        // 4. a sender without feedback does not keep an escalated rate
        const i32 before = r.idle;
        r.idle = sx_rate_sat_inc(before);
        if (p.stale_calls > 0 && before < p.stale_calls && r.idle >= p.stale_calls) {
            if (t > p.start_bps) t = p.start_bps;
            thin = false; r.over = 0; r.under = 0;
            ev |= SX_RATE_E_STALE;
        }
    } else {
        // 5. the report
        ev |= SX_RATE_E_USED;
        r.n_used++; r.idle = 0; r.flags |= SX_RATE_HAS_REPORT; r.last_ehs = ext_high_seq;
        const i32 q = fraction_lost < 0 ? 0 : (fraction_lost > 255 ? 255 : fraction_lost);
        r.last_fraction = q; r.last_rtt = rtt;
        if (rtt > 0 && rtt < r.min_rtt) r.min_rtt = rtt;
        const bool delayed = p.rtt_guard > 0 && rtt > 0 && (i64)rtt - (i64)r.min_rtt > (i64)p.rtt_guard;
        if (q > p.hi_q8) {
            r.over = t <= p.min_bps ? sx_rate_sat_inc(r.over) : 0;
            const i64 a = t - ((t * q) >> 9), b = t - p.quantum_bps;        // the factor 1 - p / 512, at least a quantum
            t = a < b ? a : b;
            ev |= SX_RATE_E_DECREASED;
        } else {
            r.over = 0;
            if (q < p.lo_q8 && !delayed && !thin) {
                const i64 s = (t * p.inc_q8) >> 8;
                t += s > p.quantum_bps ? s : (i64)p.quantum_bps;
                ev |= SX_RATE_E_INCREASED;
            } else {
                ev |= SX_RATE_E_HELD;
                if (q < p.lo_q8 && !thin) ev |= SX_RATE_E_DELAYED;          // (the delay guard was what held it)
            }
        }
        // 6. thinning: at the floor and still losing -> one description per packet; a run of clean reports ends it
        if (thin) {
            r.under = q < p.lo_q8 ? sx_rate_sat_inc(r.under) : 0;
            if (r.under >= p.thin_release) { thin = false; r.under = 0; r.over = 0; ev |= SX_RATE_E_THIN_OFF; }
        } else if (p.thin_after > 0 && r.over >= p.thin_after) {
            thin = true; r.under = 0;
            ev |= SX_RATE_E_THIN_ON;
        }
    }
    t = sx_rate_clamp64(t, p.min_bps, p.max_bps);
    t -= t % p.quantum_bps;
    r.target_bps = (i32)t;
    r.flags = (r.flags & ~SX_RATE_THIN) | (thin ? SX_RATE_THIN : 0);
    if (t != old) changed = true;
    if (changed) { ev |= SX_RATE_E_CHANGED; r.n_changed++; }
    if (thin) ev |= SX_RATE_E_THIN_ROW;
    *target = changed ? (i32)t : 0;
    *mode = thin ? 1 : 0;
    return ev;
}

// The mask rule: what packet `seq` of a row in mode `mode` sends (bit 0: MD1, bit 1: MD2 || HB), under the caller's own mask
SX_HD u8 sx_rate_mask(i32 mode, u32 seq, i32 send_in) { return (u8)((mode ? ((seq & 1) ? 2 : 1) : 3) & send_in); }

struct SxRateArgs {
    const u32* feedback;        // [n_rows][8]: solo_rtcp_feedback_t
    i32* state;                 // [n_rows][SX_RATE_STATE_WORDS]
    i32* target; u8* mode;      // [n_rows], [n_rows]
    i32* count;                 // solo_rate_count_t
    SxRateParams p;
    int n_rows;
};
struct SxRateMaskArgs {
    const u8* mode; const i32* map; const i32* seq_base; const u8* send_in; u8* send;
    int n_rows, n, n_packets; i32 first_seq;
};
// position (i, p) of a send mask call
SX_HD void sx_rate_mask_at(const SxRateMaskArgs& a, int i, int p) {
    const int row = a.map ? a.map[i] : i;
    const u32 seq = (u32)a.first_seq + (a.seq_base ? (u32)a.seq_base[i] : 0u) + (u32)p;
    const size_t at = (size_t)i * (size_t)a.n_packets + (size_t)p;
    a.send[at] = sx_rate_mask(a.mode[row], seq, a.send_in ? a.send_in[at] : 3);
}

#if defined(__HIPCC__)
// {rows, 0 ...} in front of the update kernel's atomics
__global__ void __launch_bounds__(64) solo_rate_clear_kernel(i32* count, int rows) {
    if (threadIdx.x < SX_RATE_COUNT_WORDS) count[threadIdx.x] = threadIdx.x == 0 ? rows : 0;
}
// one lane per row
__global__ void __launch_bounds__(SX_RATE_TILE) solo_rate_update_kernel(const SxRateArgs a) {
    __shared__ i32 red[4];
    const int tid = (int)threadIdx.x, i = (int)blockIdx.x * SX_RATE_TILE + tid;
    i32 ev = 0;
    if (i < a.n_rows) {
        const uint4* fp = (const uint4*)a.feedback + (size_t)i * 2;
        const uint4 f0 = fp[0], f1 = fp[1];
        uint4* sp = (uint4*)(a.state + (size_t)i * SX_RATE_STATE_WORDS);
        const uint4 q0 = sp[0], q1 = sp[1], q2 = sp[2];     // (words 0 .. 11: the live words and one that goes back as it came)
        SxRateRow r;
        r.flags = (i32)q0.x; r.target_bps = (i32)q0.y; r.last_ehs = q0.z; r.min_rtt = (i32)q0.w;
        r.idle = (i32)q1.x; r.over = (i32)q1.y; r.under = (i32)q1.z; r.n_used = q1.w;
        r.n_changed = q2.x; r.last_fraction = (i32)q2.y; r.last_rtt = (i32)q2.z;
        i32 target, mode;
        ev = sx_rate_step(r, a.p, (i32)f0.x, (i32)f0.y, f0.w, (i32)f1.w, &target, &mode);
        sp[0] = make_uint4((u32)r.flags, (u32)r.target_bps, r.last_ehs, (u32)r.min_rtt);
        sp[1] = make_uint4((u32)r.idle, (u32)r.over, (u32)r.under, r.n_used);
        sp[2] = make_uint4(r.n_changed, (u32)r.last_fraction, (u32)r.last_rtt, q2.w);
        a.target[i] = target;
        a.mode[i] = (u8)mode;
    }
    i32 mine = 0;
#pragma unroll
    for (int g = 0; g < (SX_RATE_N_EVENTS + 2) / 3; g++) {
        const i32 s = wg_sum(((ev >> (3 * g)) & 1) | (((ev >> (3 * g + 1)) & 1) << 10) | (((ev >> (3 * g + 2)) & 1) << 20), red);
        if (tid / 3 == g) mine = (s >> (10 * (tid % 3))) & 1023;
    }
    if (tid < SX_RATE_N_EVENTS && mine) atomicAdd(a.count + 1 + tid, mine);
}
// One lane per (position, packet).  The call has no object that could keep a verdict word, and a word of the library's would be shared
// by calls in flight on different streams: every workgroup checks the list itself (n / 256 loads a lane, one wg_sum) and leaves before
// it writes anything if the list is not strictly increasing inside [0, n_rows).
__global__ void __launch_bounds__(SX_RATE_TILE) solo_rate_send_mask_kernel(const SxRateMaskArgs a) {
    __shared__ i32 red[4];
    if (a.map) {
        i32 bad = 0;
        for (int k = (int)threadIdx.x; k < a.n; k += SX_RATE_TILE) {
            const i32 v = a.map[k];
            if (v < 0 || v >= a.n_rows || (k > 0 && a.map[k - 1] >= v)) bad = 1;
        }
        if (wg_sum(bad, red)) return;
    }
    const long long idx = (long long)blockIdx.x * SX_RATE_TILE + threadIdx.x;
    if (idx >= (long long)a.n * a.n_packets) return;
    sx_rate_mask_at(a, (int)(idx / a.n_packets), (int)(idx % a.n_packets));
}
static inline hipError_t solo_rate_update_launch(const SxRateArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(solo_rate_clear_kernel, dim3(1), dim3(64), 0, s, a.count, a.n_rows);
    hipLaunchKernelGGL(solo_rate_update_kernel, dim3((unsigned)((a.n_rows + SX_RATE_TILE - 1) / SX_RATE_TILE)), dim3(SX_RATE_TILE), 0, s, a);
    return hipGetLastError();
}
static inline hipError_t solo_rate_send_mask_launch(const SxRateMaskArgs& a, hipStream_t s) {
    const long long lanes = (long long)a.n * a.n_packets;
    hipLaunchKernelGGL(solo_rate_send_mask_kernel, dim3((unsigned)((lanes + SX_RATE_TILE - 1) / SX_RATE_TILE)), dim3(SX_RATE_TILE), 0, s, a);
    return hipGetLastError();
}
#else
// Host forms of the launches (tests): every row through sx_rate_step, every position through sx_rate_mask_at
static inline void sx_rate_update_host(const SxRateArgs& a) {
    for (int w = 0; w < SX_RATE_COUNT_WORDS; w++) a.count[w] = w == 0 ? a.n_rows : 0;
    for (int i = 0; i < a.n_rows; i++) {
        const u32* f = a.feedback + (size_t)i * 8;
        SxRateRow* r = (SxRateRow*)(a.state + (size_t)i * SX_RATE_STATE_WORDS);
        i32 target, mode;
        const i32 ev = sx_rate_step(*r, a.p, (i32)f[0], (i32)f[1], f[3], (i32)f[7], &target, &mode);
        a.target[i] = target;
        a.mode[i] = (u8)mode;
        for (int k = 0; k < SX_RATE_N_EVENTS; k++) a.count[1 + k] += (ev >> k) & 1;
    }
}
// -> false: the list is not strictly increasing inside [0, n_rows), nothing is written
static inline bool sx_rate_send_mask_host(const SxRateMaskArgs& a) {
    if (!sx_map_ok(a.map, a.n, a.n_rows)) return false;
    for (int i = 0; i < a.n; i++)
        for (int p = 0; p < a.n_packets; p++) sx_rate_mask_at(a, i, p);
    return true;
}
#endif

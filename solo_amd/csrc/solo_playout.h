// solo_playout.h -- adaptive play-out delay control: which stream plays one packet, which is stretched 1 -> 2, which is shortened 2 -> 1,
// decided on the device from the receive reports with a state record per row, and the one row of audio per stream that results
// (solo_playout_plan / _gather / _render / _tick, include/solo_mi355x.h, whose comment is the reference for the rule).
//
// The state record of a row is 128 bytes = 32 words:
//     0 run   1 held   2 cum   3 cool   4 age   5 late_prev (uint32)   6 pos (next ring slot, 0 .. 31)   7 zero
//     8 .. 23  the ring: 32 observations of int16, slot j in half (j & 1) of word 8 + (j >> 1); -32768 = none     24 .. 31 zero
// and behind it, in a store of its own, one packet of PCM: the held packet.
//
// The cuts.
//   plan     ONE LANE per row, the ring in registers.  A row's decision is serial (observation -> ring -> quantile -> rule) and small: the
//            quantile is at most the 4th smallest of at most 32 values, which one pass of a four-deep sorted insert finds (7 min / max
//            per slot, the slots addressed by unrolled constants, so nothing is indexed dynamically and nothing goes to scratch).  A group of
//            lanes per row would spread 32 values over the lanes and pay lane-crossing selects for a dozen instructions of work; a lane per
//            row also is the geometry of the compaction tile.  The record is read and written as 16-byte quads.
//   compact  the three lists in row order with the workgroup scan of solo_wave.h, three flags side by side (solo_recv_compact_kernel's
//            scheme: a tile counts the flags in front of it itself).  It also leaves, per row, the position of the row in its list:
//            what render needs to find the row's decoded audio.
//   gather   one wavefront per STRETCH row, 16-byte copies.
//   render   one wavefront per row: the largest splice cost of the row (wave max), the outcome, the row of d_heard and the held store by
//            16-byte copies, lane 0 finishes the state.  The per-outcome count is a pass of its own over d_outcome (one workgroup,
//            wg_sum): no atomics.
//
// Everything outside the kernels compiles for the host as well (tests/playout_host.cpp walks the rows through the very functions of the
// kernels; tests/test_playout_model.py compares them with the independent model of tests/playout_model.py).
#pragma once
#include <stddef.h>
#include <string.h>
#include "solo_wave.h"          // wg_sum, wg_scan_incl
#include "solo_stream_ctl.h"    // sx_map_refused, the list launches
#include "solo_timescale.h"     // SxTsX8, SX_TS_MAX_BLOCKS

#define SX_PO_TILE 256          // rows per workgroup of the plan and of the compaction = its lanes (wg_sum / wg_scan_incl are for 256)

#define SX_PO_STATE_WORDS 32
#define SX_PO_RING 32                                       // slots of the ring = the longest window
#define SX_PO_NONE (-32768)
#define SX_PO_CUM_MAX 16000                                 // |cum| saturates here: v = s - cum stays an int16
#define SX_PO_SLACK_MAX 1000
#define SX_PO_MAX_TOLERATE 3
#define SX_PO_MAX_SLACK_PARAM 64
#define SX_PO_MAX_COOLDOWN 1000
#define SX_PO_MAX_L 1920

#define SX_PO_ACT_IDLE 0
#define SX_PO_ACT_NORMAL 1
#define SX_PO_ACT_HELD 2
#define SX_PO_ACT_STRETCH 3
#define SX_PO_ACT_ACCEL 4
#define SX_PO_ACT_ACCEL_FORCED 5

#define SX_PO_OUT_IDLE SOLO_PLAYOUT_IDLE
#define SX_PO_OUT_NORMAL SOLO_PLAYOUT_NORMAL
#define SX_PO_OUT_HELD SOLO_PLAYOUT_HELD
#define SX_PO_OUT_STRETCH SOLO_PLAYOUT_STRETCH
#define SX_PO_OUT_STRETCH_GATED SOLO_PLAYOUT_STRETCH_GATED
#define SX_PO_OUT_ACCEL SOLO_PLAYOUT_ACCEL
#define SX_PO_OUT_ACCEL_GATED SOLO_PLAYOUT_ACCEL_GATED
#define SX_PO_OUT_ACCEL_FORCED SOLO_PLAYOUT_ACCEL_FORCED
#define SX_PO_N_OUTCOMES 8

typedef solo_playout_params_t SxPoParams;
// The three counts are the public records with what those do not say: the 16-byte alignment the interface asks of the caller (the kernels
// store whole records), and the outcomes as an array indexed by the SOLO_PLAYOUT_* code.
struct alignas(16) SxPoPlanCount { i32 n_one, n_two, n_stretch, listed; };
struct alignas(16) SxPoRenderCount { i32 outcome[SX_PO_N_OUTCOMES]; };
struct SxPoCount { SxPoPlanCount plan; SxPoRenderCount render; };
static_assert(sizeof(SxPoParams) == 32 && sizeof(SxPoPlanCount) == 16 && sizeof(SxPoRenderCount) == 32 && sizeof(SxPoCount) == 48, "solo_playout_* layout");
// ... and agree with them field by field: every public field at the twin's word, every outcome's field at the index of its code
#define SX_PO_SAME(pub, twin, f) (offsetof(pub, f) == offsetof(twin, f) && sizeof(((pub*)0)->f) == sizeof(((twin*)0)->f))
#define SX_PO_OUTCOME(f, code) (offsetof(solo_playout_render_count_t, f) == offsetof(SxPoRenderCount, outcome) + sizeof(i32) * (code))
static_assert(SX_PO_SAME(solo_playout_plan_count_t, SxPoPlanCount, n_one) && SX_PO_SAME(solo_playout_plan_count_t, SxPoPlanCount, n_two) &&
              SX_PO_SAME(solo_playout_plan_count_t, SxPoPlanCount, n_stretch) && SX_PO_SAME(solo_playout_plan_count_t, SxPoPlanCount, listed) &&
              sizeof(solo_playout_plan_count_t) == sizeof(SxPoPlanCount) && alignof(SxPoPlanCount) == 16, "solo_playout_plan_count_t, field by field");
static_assert(SX_PO_OUTCOME(idle, SOLO_PLAYOUT_IDLE) && SX_PO_OUTCOME(normal, SOLO_PLAYOUT_NORMAL) && SX_PO_OUTCOME(held, SOLO_PLAYOUT_HELD) &&
              SX_PO_OUTCOME(stretch, SOLO_PLAYOUT_STRETCH) && SX_PO_OUTCOME(stretch_gated, SOLO_PLAYOUT_STRETCH_GATED) &&
              SX_PO_OUTCOME(accel, SOLO_PLAYOUT_ACCEL) && SX_PO_OUTCOME(accel_gated, SOLO_PLAYOUT_ACCEL_GATED) &&
              SX_PO_OUTCOME(accel_forced, SOLO_PLAYOUT_ACCEL_FORCED) && SOLO_PLAYOUT_ACCEL_FORCED + 1 == SX_PO_N_OUTCOMES &&
              sizeof(solo_playout_render_count_t) == sizeof(SxPoRenderCount) && alignof(SxPoRenderCount) == 16, "solo_playout_render_count_t, field by field");
static_assert(SX_PO_SAME(solo_playout_count_t, SxPoCount, plan) && SX_PO_SAME(solo_playout_count_t, SxPoCount, render) &&
              sizeof(solo_playout_count_t) == sizeof(SxPoCount) && alignof(SxPoCount) == 16, "solo_playout_count_t, field by field");
#undef SX_PO_SAME
#undef SX_PO_OUTCOME

struct SxPoCtl { i32 run, held, cum, cool, age; u32 late_prev; i32 pos, zero; };
struct SxPoRow { SxPoCtl c; u32 ring[SX_PO_RING / 2]; };    // words 0 .. 23 of a record, in registers
static_assert(sizeof(SxPoRow) == 96, "the live part of a state record");

static inline bool sx_po_params_ok(const SxPoParams* p) {
    return p && p->start_ready >= 1 && p->max_span >= 0 && p->window >= 1 && p->window <= SX_PO_RING && p->tolerate >= 0 && p->tolerate <= SX_PO_MAX_TOLERATE &&
           p->lo >= 0 && p->lo <= p->hi && p->hi <= SX_PO_MAX_SLACK_PARAM && p->cooldown >= 0 && p->cooldown <= SX_PO_MAX_COOLDOWN;
}
static inline bool sx_po_geometry_ok(i32 n_rows, i32 L) {
    return n_rows > 0 && L > 0 && L <= SX_PO_MAX_L && L % 8 == 0 && (i64)n_rows * (2 * (i64)L) < ((i64)1 << 31);
}
// (the name the host build of tests/playout_host.cpp asks the host-list rule by)
static inline bool sx_po_list_ok(const i32* rows, i32 n, i32 n_rows) { return sx_list_ok(rows, n, n_rows); }

// what the host checks of a call before it enqueues anything (solo_api.hip; the host build of the tests asks the same functions)
static inline bool sx_po_rows_ok(i32 n_rows, const void* rows, i32 n) { return n > 0 && n <= n_rows && (rows || n == n_rows); }
static inline bool sx_po_plan_call_ok(i32 n_rows, const void* reports, const void* rows, i32 n, i32 depth, const SxPoParams* p, const void* action,
                                      const void* one, const void* two, const void* spos, const void* count) {
    if (!reports || !action || !one || !two || !spos || !count || !sx_po_params_ok(p) || !sx_po_rows_ok(n_rows, rows, n) || depth <= 0) return false;
    return !((uintptr_t)reports & 15) && !((uintptr_t)count & 15);
}
static inline bool sx_po_gather_call_ok(i32 n_rows, const void* pcm_one, i32 n_one, const void* spos, i32 n_stretch, const void* out) {
    if (!pcm_one || !spos || !out || n_one <= 0 || n_one > n_rows || n_stretch <= 0 || n_stretch > n_one) return false;
    return !((uintptr_t)pcm_one & 15) && !((uintptr_t)out & 15);
}
static inline bool sx_po_render_call_ok(i32 n_rows, i32 L, const void* rows, i32 n, const SxPoParams* p, i32 block, const void* action, i32 n_one, i32 n_two,
                                        i32 n_stretch, const void* pcm_one, const void* st_one, const void* pcm_two, const void* st_two, const void* ts_s,
                                        const void* cost_s, const void* ts_a, const void* cost_a, const void* heard, const void* outcome, const void* status,
                                        const void* count) {
    if (!action || !heard || !outcome || !status || !sx_po_params_ok(p) || !sx_po_rows_ok(n_rows, rows, n)) return false;
    if (block <= 0 || L % block || 2 * (L / block) > SX_TS_MAX_BLOCKS) return false;
    if (n_one < 0 || n_two < 0 || n_stretch < 0 || n_stretch > n_one || (i64)n_one + n_two > n) return false;
    if ((n_one && (!pcm_one || !st_one)) || (n_two && (!pcm_two || !st_two || !ts_a || !cost_a)) || (n_stretch && (!ts_s || !cost_s))) return false;
    return !(((uintptr_t)heard | (uintptr_t)pcm_one | (uintptr_t)pcm_two | (uintptr_t)ts_s | (uintptr_t)ts_a | (uintptr_t)count) & 15);
}
// ... of a tick; the handle's facts: has a ring, tracking on, streams, ring depth, packet samples, sample rate
static inline bool sx_po_tick_call_ok(i32 n_rows, i32 L, bool ring, bool tracking, i32 h_streams, i32 h_depth, i32 h_L, i32 h_fs, const void* rows, i32 n,
                                      const SxPoParams* p, const void* heard, const void* outcome, const void* status, const void* count) {
    if (!ring || !tracking || h_streams != n_rows || h_depth < 2 || h_L != L) return false;
    const i32 H = h_fs / 200;
    if ((H != 80 && H != 160) || L % H || L > SX_TS_MAX_L) return false;
    if (!sx_po_params_ok(p) || !heard || !outcome || !status || !count || !sx_po_rows_ok(n_rows, rows, n)) return false;
    return !(((uintptr_t)heard | (uintptr_t)count) & 15);
}

SX_HD i32 sx_po_ring_get(const u32 (&ring)[SX_PO_RING / 2], int j) { return (i32)(i16)(u16)(ring[j >> 1] >> (16 * (j & 1))); }

// One row of the plan: observation, ring, quantile, decision.  ready / span / late / margin_min: the row's report; depth: the ring depth
// of the handle (margin_min == depth is "no arrival").  -> the action
SX_HD i32 sx_po_plan_row(SxPoRow& r, const SxPoParams& p, i32 ready, i32 span, u32 late, i32 margin_min, i32 depth) {
    const bool over = p.max_span > 0 && span >= p.max_span;
    if (!r.c.run) {
        if (ready < p.start_ready && !over) return SX_PO_ACT_IDLE;
#pragma unroll
        for (int k = 0; k < SX_PO_RING / 2; k++) r.ring[k] = 0x80008000u;
        r.c.run = 1; r.c.held = 0; r.c.cum = 0; r.c.cool = 0; r.c.age = 0; r.c.late_prev = late; r.c.pos = 0; r.c.zero = 0;
        return SX_PO_ACT_NORMAL;
    }
    // the observation: the slack of this tick's arrivals, relative to the delay added so far
    const u32 dl = late - r.c.late_prev;
    r.c.late_prev = late;
    i32 v = SX_PO_NONE;
    if (dl > 0) v = -1 - r.c.cum;
    else if (margin_min < depth) v = sx_min(sx_max(margin_min + (r.c.held != 0), -1), SX_PO_SLACK_MAX) - r.c.cum;
    const int pos = r.c.pos & (SX_PO_RING - 1);
    {
        const u32 half = (u32)(u16)(i16)v << (16 * (pos & 1)), keep = 0xFFFF0000u >> (16 * (pos & 1));
#pragma unroll
        for (int k = 0; k < SX_PO_RING / 2; k++) r.ring[k] = k == (pos >> 1) ? ((r.ring[k] & keep) | half) : r.ring[k];
    }
    r.c.pos = (pos + 1) & (SX_PO_RING - 1);
    r.c.age = sx_min(r.c.age + 1, p.window);
    // the (tolerate + 1)-th smallest value among the last `age` slots: a four-deep sorted insert
    const i32 BIG = 0x7FFFFFFF;
    i32 b0 = BIG, b1 = BIG, b2 = BIG, b3 = BIG, have = 0;
#pragma unroll
    for (int j = 0; j < SX_PO_RING; j++) {
        i32 x = sx_po_ring_get(r.ring, j);
        const bool in = ((pos - j) & (SX_PO_RING - 1)) < r.c.age && x != SX_PO_NONE;
        have += in;
        x = in ? x : BIG;
        i32 t;
        t = sx_min(b0, x); x = sx_max(b0, x); b0 = t;
        t = sx_min(b1, x); x = sx_max(b1, x); b1 = t;
        t = sx_min(b2, x); x = sx_max(b2, x); b2 = t;
        b3 = sx_min(b3, x);
    }
    const bool def = have > p.tolerate;
    const i32 q = p.tolerate == 0 ? b0 : (p.tolerate == 1 ? b1 : (p.tolerate == 2 ? b2 : b3));
    const i32 e = def ? q + r.c.cum : 0;
    // the decision: the first rule that applies
    if (r.c.held) { r.c.cool = sx_max(r.c.cool - 1, 0); return SX_PO_ACT_HELD; }
    if (over) return SX_PO_ACT_ACCEL_FORCED;
    if (r.c.cool > 0) { r.c.cool--; return SX_PO_ACT_NORMAL; }
    if (def && e < p.lo && ready >= 1 && (p.max_span <= 0 || span + 1 < p.max_span)) return SX_PO_ACT_STRETCH;
    if (r.c.age >= p.window && def && e > p.hi && ready >= 2) return SX_PO_ACT_ACCEL;
    return SX_PO_ACT_NORMAL;
}

struct SxPoPlanArgs {
    const u32* reports;         // [n][16]: solo_recv_report_t
    i32* state;                 // [n_rows][SX_PO_STATE_WORDS]
    const i32* map;             // the listed rows, or NULL
    i32* action;                // [n]
    SxPoParams p;
    int n, depth;
};
// the three flags of an action: in d_one, in d_two, a STRETCH row
SX_HD void sx_po_flags(i32 act, i32* f_one, i32* f_two, i32* f_st) {
    *f_one = act == SX_PO_ACT_NORMAL || act == SX_PO_ACT_STRETCH;
    *f_two = act == SX_PO_ACT_ACCEL || act == SX_PO_ACT_ACCEL_FORCED;
    *f_st = act == SX_PO_ACT_STRETCH;
}

struct SxPoRenderArgs {
    i32* state; i16* held;      // [n_rows][32], [n_rows][L]
    const i32* map; const i32* action; const i32* slot; const i32* sslot;                   // [n]: the plan's
    const i16* pcm_one; const i32* st_one;                  // [n_one][1][L], [n_one]: solo_recv_decode_streams(d_one, 1)
    const i16* pcm_two; const i32* st_two;                  // [n_two][2][L], [n_two]
    const i16* ts_s; const i32* cost_s;                     // [n_stretch][2][L], [n_stretch][2 M]: solo_timescale 1 -> 2
    const i16* ts_a; const i32* cost_a;                     // [n_two][1][L], [n_two][M]: solo_timescale 2 -> 1
    i16* heard; i32* outcome; i32* status;                  // [n][L], [n], [n]
    int n, n_one, n_two, n_stretch, L, M, cooldown, cost_gate;
};

// One row of the render: what one wavefront does
SX_HD void sx_po_render_row(const SxPoRenderArgs& a, int i) {
    const int s = a.map ? a.map[i] : i, L = a.L;
    i32 act = SX_UNI(a.action[i]);                          // (wave-uniform: the wave reductions below run with every lane)
    const i32 k = SX_UNI(a.slot[i]), j = SX_UNI(a.sslot[i]);
    // (positions outside the buffers the caller brought -- actions that are not the last plan's -- are played as IDLE rows)
    if ((act == SX_PO_ACT_NORMAL || act == SX_PO_ACT_STRETCH) && (k < 0 || k >= a.n_one)) act = SX_PO_ACT_IDLE;
    if ((act == SX_PO_ACT_ACCEL || act == SX_PO_ACT_ACCEL_FORCED) && (k < 0 || k >= a.n_two)) act = SX_PO_ACT_IDLE;
    if (act == SX_PO_ACT_STRETCH && (j < 0 || j >= a.n_stretch)) act = SX_PO_ACT_IDLE;
    if (act < 0 || act > SX_PO_ACT_ACCEL_FORCED) act = SX_PO_ACT_IDLE;
    i32* st = a.state + (size_t)s * SX_PO_STATE_WORDS;
    i16* held = a.held + (size_t)s * (size_t)L;
    const i16* src = (const i16*)0;     // what is heard; NULL: silence
    const i16* keep = (const i16*)0;    // what goes to the held store
    i32 out = SX_PO_OUT_IDLE, status = 0, new_held = -1, dcum = 0, cool_set = 0;
    if (act == SX_PO_ACT_NORMAL) { out = SX_PO_OUT_NORMAL; src = a.pcm_one + (size_t)k * L; status = a.st_one[k]; }
    else if (act == SX_PO_ACT_HELD) { out = SX_PO_OUT_HELD; src = held; new_held = 0; }
    else if (act == SX_PO_ACT_STRETCH) {
        i32 mx = 0;
        SX_PAR(m, 2 * a.M) mx = sx_max(mx, a.cost_s[(size_t)j * (2 * a.M) + m]);
        mx = wv_max(mx);
        status = a.st_one[k];
        if (a.cost_gate > 0 && mx > a.cost_gate) { out = SX_PO_OUT_STRETCH_GATED; src = a.pcm_one + (size_t)k * L; }
        else { out = SX_PO_OUT_STRETCH; src = a.ts_s + (size_t)j * 2 * L; keep = src + L; new_held = 1; dcum = 1; cool_set = 1; }
    } else if (act == SX_PO_ACT_ACCEL || act == SX_PO_ACT_ACCEL_FORCED) {
        i32 mx = 0;
        SX_PAR(m, a.M) mx = sx_max(mx, a.cost_a[(size_t)k * a.M + m]);
        mx = wv_max(mx);
        status = a.st_two[k];
        if (act == SX_PO_ACT_ACCEL && a.cost_gate > 0 && mx > a.cost_gate) {
            out = SX_PO_OUT_ACCEL_GATED; src = a.pcm_two + (size_t)k * 2 * L; keep = src + L; new_held = 1;
        } else {
            out = act == SX_PO_ACT_ACCEL ? SX_PO_OUT_ACCEL : SX_PO_OUT_ACCEL_FORCED; src = a.ts_a + (size_t)k * L; dcum = -1; cool_set = 1;
        }
    }
    SxTsX8* dst = (SxTsX8*)(a.heard + (size_t)i * L);
    SX_PAR(ch, L >> 3) {
        SxTsX8 v;
        if (src) v = ((const SxTsX8*)src)[ch];
        else { v.d[0] = v.d[1] = v.d[2] = v.d[3] = 0; }
        dst[ch] = v;
        if (keep) ((SxTsX8*)held)[ch] = ((const SxTsX8*)keep)[ch];
    }
    if (SX_LANE == 0) {
        if (new_held >= 0) st[1] = new_held;
        if (dcum) st[2] = sx_max(sx_min(st[2] + dcum, SX_PO_CUM_MAX), -SX_PO_CUM_MAX);
        if (cool_set) st[3] = a.cooldown;
        a.outcome[i] = out;
        a.status[i] = status;
    }
}

// bytes per row of a state blob (solo_playout_get_state / _set_state): the record, then the held packet
SX_HD size_t sx_po_blob_row_words(int L) { return SX_PO_STATE_WORDS + (size_t)L / 2; }

#if defined(__HIPCC__)
// one lane per row
__global__ void __launch_bounds__(SX_PO_TILE) solo_playout_plan_kernel(const SxPoPlanArgs a, const u32* verdict) {
    if (sx_map_refused(a.map, verdict)) return;
    const int i = (int)blockIdx.x * SX_PO_TILE + (int)threadIdx.x;
    if (i >= a.n) return;
    const int s = a.map ? a.map[i] : i;
    const uint4* rp = (const uint4*)a.reports + (size_t)i * 4;
    const uint4 r0 = rp[0], r1 = rp[1], r3 = rp[3];
    uint4* sp = (uint4*)(a.state + (size_t)s * SX_PO_STATE_WORDS);
    SxPoRow r;
    uint4 q[6];
#pragma unroll
    for (int k = 0; k < 6; k++) q[k] = sp[k];
    r.c.run = (i32)q[0].x; r.c.held = (i32)q[0].y; r.c.cum = (i32)q[0].z; r.c.cool = (i32)q[0].w;
    r.c.age = (i32)q[1].x; r.c.late_prev = q[1].y; r.c.pos = (i32)q[1].z; r.c.zero = (i32)q[1].w;
#pragma unroll
    for (int k = 0; k < 4; k++) { r.ring[4 * k] = q[2 + k].x; r.ring[4 * k + 1] = q[2 + k].y; r.ring[4 * k + 2] = q[2 + k].z; r.ring[4 * k + 3] = q[2 + k].w; }
    const i32 act = sx_po_plan_row(r, a.p, (i32)r0.w, (i32)r1.x, r1.w, (i32)r3.w, a.depth);
    a.action[i] = act;
    if (act == SX_PO_ACT_IDLE) return;                      // (an idle row's record did not move)
    q[0] = make_uint4((u32)r.c.run, (u32)r.c.held, (u32)r.c.cum, (u32)r.c.cool);
    q[1] = make_uint4((u32)r.c.age, r.c.late_prev, (u32)r.c.pos, (u32)r.c.zero);
#pragma unroll
    for (int k = 0; k < 4; k++) q[2 + k] = make_uint4(r.ring[4 * k], r.ring[4 * k + 1], r.ring[4 * k + 2], r.ring[4 * k + 3]);
#pragma unroll
    for (int k = 0; k < 6; k++) sp[k] = q[k];
}

// the three lists in row order; slot[i] / sslot[i]: where row i stands in d_one or d_two / among the STRETCH rows (-1: in none)
__global__ void __launch_bounds__(SX_PO_TILE) solo_playout_compact_kernel(const i32* __restrict__ action, const i32* __restrict__ map, int n,
                                                                           i32* __restrict__ one, i32* __restrict__ two, i32* __restrict__ spos,
                                                                           i32* __restrict__ slot, i32* __restrict__ sslot, SxPoPlanCount* count,
                                                                           const u32* verdict) {
    __shared__ i32 red[4], part[3][4];
    if (sx_map_refused(map, verdict)) {
        if (blockIdx.x == 0 && threadIdx.x == 0) count->n_one = -1;
        return;
    }
    const int tid = (int)threadIdx.x, t0 = (int)blockIdx.x * SX_PO_TILE;
    i32 b1 = 0, b2 = 0, b3 = 0;
    for (int i = tid; i < t0; i += SX_PO_TILE) {
        i32 f1, f2, f3;
        sx_po_flags(action[i], &f1, &f2, &f3);
        b1 += f1; b2 += f2; b3 += f3;
    }
    b1 = wg_sum(b1, red); b2 = wg_sum(b2, red); b3 = wg_sum(b3, red);
    const int i = t0 + tid;
    i32 f[3] = {0, 0, 0};
    if (i < n) sx_po_flags(action[i], &f[0], &f[1], &f[2]);
    i32 v[3] = {f[0], f[1], f[2]};
    wg_scan_incl(v, part);
    const i32 k1 = b1 + v[0] - f[0], k2 = b2 + v[1] - f[1], k3 = b3 + v[2] - f[2];       // (each below n: there are at most n flags)
    if (i < n) {
        const i32 s = map ? map[i] : i;
        if (f[0]) one[k1] = s;
        if (f[1]) two[k2] = s;
        if (f[2]) spos[k3] = k1;
        slot[i] = f[0] ? k1 : (f[1] ? k2 : -1);
        sslot[i] = f[2] ? k3 : -1;
    }
    if (i == n - 1) { SxPoPlanCount c; c.n_one = k1 + f[0]; c.n_two = k2 + f[1]; c.n_stretch = k3 + f[2]; c.listed = n; *count = c; }
}

// row spos[j] of the one-packet decode output -> row j of the time scaler's input; one wavefront per STRETCH row
__global__ void __launch_bounds__(64) solo_playout_gather_kernel(const i16* __restrict__ pcm_one, const i32* __restrict__ spos, int n_one, int L,
                                                                 i16* __restrict__ out) {
    const int j = (int)blockIdx.x, k = spos[j];
    if (k < 0 || k >= n_one) return;
    const SxTsX8* src = (const SxTsX8*)(pcm_one + (size_t)k * L);
    SxTsX8* dst = (SxTsX8*)(out + (size_t)j * L);
    SX_PAR(ch, L >> 3) dst[ch] = src[ch];
}

// one wavefront per row
__global__ void __launch_bounds__(64) solo_playout_render_kernel(const SxPoRenderArgs a, const u32* verdict) {
    if (sx_map_refused(a.map, verdict)) return;
    sx_po_render_row(a, (int)blockIdx.x);
}
// how many rows had each outcome: one workgroup over d_outcome
__global__ void __launch_bounds__(SX_PO_TILE) solo_playout_count_kernel(const i32* __restrict__ outcome, int n, const i32* map, SxPoRenderCount* count,
                                                                         const u32* verdict) {
    __shared__ i32 red[4];
    if (sx_map_refused(map, verdict)) {
        if (threadIdx.x == 0) count->outcome[0] = -1;
        return;
    }
    i32 c[SX_PO_N_OUTCOMES];
#pragma unroll
    for (int o = 0; o < SX_PO_N_OUTCOMES; o++) c[o] = 0;
    for (int i = (int)threadIdx.x; i < n; i += SX_PO_TILE) {
        const i32 v = outcome[i];
#pragma unroll
        for (int o = 0; o < SX_PO_N_OUTCOMES; o++) c[o] += v == o;
    }
#pragma unroll
    for (int o = 0; o < SX_PO_N_OUTCOMES; o++) c[o] = wg_sum(c[o], red);
    if (threadIdx.x < SX_PO_N_OUTCOMES) {
        i32 mine = 0;
#pragma unroll
        for (int o = 0; o < SX_PO_N_OUTCOMES; o++) mine = (int)threadIdx.x == o ? c[o] : mine;
        count->outcome[threadIdx.x] = mine;
    }
}

static inline hipError_t solo_playout_plan_launch(const SxPoPlanArgs& a, i32* one, i32* two, i32* spos, i32* slot, i32* sslot, SxPoPlanCount* count,
                                                  const u32* verdict, hipStream_t s) {
    const unsigned tiles = (unsigned)((a.n + SX_PO_TILE - 1) / SX_PO_TILE);
    hipLaunchKernelGGL(solo_playout_plan_kernel, dim3(tiles), dim3(SX_PO_TILE), 0, s, a, verdict);
    hipLaunchKernelGGL(solo_playout_compact_kernel, dim3(tiles), dim3(SX_PO_TILE), 0, s, a.action, a.map, a.n, one, two, spos, slot, sslot, count, verdict);
    return hipGetLastError();
}
static inline hipError_t solo_playout_gather_launch(const i16* pcm_one, const i32* spos, int n_one, int n_stretch, int L, i16* out, hipStream_t s) {
    hipLaunchKernelGGL(solo_playout_gather_kernel, dim3((unsigned)n_stretch), dim3(64), 0, s, pcm_one, spos, n_one, L, out);
    return hipGetLastError();
}
static inline hipError_t solo_playout_render_launch(const SxPoRenderArgs& a, SxPoRenderCount* count, const u32* verdict, hipStream_t s) {
    hipLaunchKernelGGL(solo_playout_render_kernel, dim3((unsigned)a.n), dim3(64), 0, s, a, verdict);
    if (count) hipLaunchKernelGGL(solo_playout_count_kernel, dim3(1), dim3(SX_PO_TILE), 0, s, a.outcome, a.n, a.map, count, verdict);
    return hipGetLastError();
}
#else
// Host form of the plan (tests): the rows one by one through sx_po_plan_row, then the lists as the compaction leaves them.
// -> false: the list is not strictly increasing inside [0, n_rows), nothing but count->n_one = -1 is written
static inline bool sx_po_plan_host(const SxPoPlanArgs& a, int n_rows, i32* one, i32* two, i32* spos, i32* slot, i32* sslot, SxPoPlanCount* count) {
    if (!sx_map_ok(a.map, a.n, n_rows)) { count->n_one = -1; return false; }
    i32 k1 = 0, k2 = 0, k3 = 0;
    for (int i = 0; i < a.n; i++) {
        const int s = a.map ? a.map[i] : i;
        const u32* rp = a.reports + (size_t)i * 16;
        i32* sp = a.state + (size_t)s * SX_PO_STATE_WORDS;
        SxPoRow r;
        memcpy(&r, sp, sizeof(r));
        const i32 act = sx_po_plan_row(r, a.p, (i32)rp[3], (i32)rp[4], rp[7], (i32)rp[15], a.depth);
        a.action[i] = act;
        if (act != SX_PO_ACT_IDLE) memcpy(sp, &r, sizeof(r));
        i32 f1, f2, f3;
        sx_po_flags(act, &f1, &f2, &f3);
        if (f1) one[k1] = s;
        if (f2) two[k2] = s;
        if (f3) spos[k3] = k1;
        slot[i] = f1 ? k1 : (f2 ? k2 : -1);
        sslot[i] = f3 ? k3 : -1;
        k1 += f1; k2 += f2; k3 += f3;
    }
    count->n_one = k1; count->n_two = k2; count->n_stretch = k3; count->listed = a.n;
    return true;
}
static inline void sx_po_gather_host(const i16* pcm_one, const i32* spos, int n_one, int n_stretch, int L, i16* out) {
    for (int j = 0; j < n_stretch; j++)
        if (spos[j] >= 0 && spos[j] < n_one) memcpy(out + (size_t)j * L, pcm_one + (size_t)spos[j] * L, (size_t)L * sizeof(i16));
}
// ... of the render and its count
static inline bool sx_po_render_host(const SxPoRenderArgs& a, int n_rows, SxPoRenderCount* count) {
    if (!sx_map_ok(a.map, a.n, n_rows)) { if (count) count->outcome[0] = -1; return false; }
    for (int i = 0; i < a.n; i++) sx_po_render_row(a, i);
    if (count) {
        for (int o = 0; o < SX_PO_N_OUTCOMES; o++) count->outcome[o] = 0;
        for (int i = 0; i < a.n; i++) count->outcome[a.outcome[i]]++;
    }
    return true;
}
#endif

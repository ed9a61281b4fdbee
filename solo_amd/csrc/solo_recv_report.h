// solo_recv_report.h -- the read side of the receiver staging ring (solo_recv.h): what is queued for a stream, what became of its
// arrivals and of its played packets, and which streams are ready to play (solo_recv_report, solo_recv_track, include/solo_mi355x.h).
//
// The ring knows a stream by its D length words (one per entry; low half = bytes in slot A, high half = bytes in slot B) and its
// play-out position p.  Play-out clears what it played, so every non-empty entry belongs to exactly one sequence number of
// [p, p + D): entry e holds sequence number p + ((e - p mod D) mod D).  All queue fields come from the length words alone:
//
//     queued    non-empty entries                     complete  entries with both descriptions
//     ready     length of the run of non-empty entries that starts at p
//     span      1 + (highest queued sequence number - p), 0 when the queue is empty
//     head      entry p in d_recv format: bit 0 MD1 queued, bit 1 MD2 || HB queued
//
// Cut of the report kernel.  A stream is read by a GROUP of G lanes, G = the power of two at or above min(D, 64): the lanes load the
// entries in PHYSICAL order (coalesced; a stream's words are contiguous), two ballots turn "slot A filled" / "slot B filled" into bit
// masks, and the group's bits are cut out of them.  64 / G streams share a wavefront -- eight at the default depth of 8 --, a queue
// deeper than 64 is walked 64 entries at a time by a whole wavefront.  The rotation by p mod D never touches the data: the part of a
// mask at or above p mod D is the front of the window, the part below it is the back, and first-empty / last-filled of either part are
// one count-trailing / count-leading-zeros each (sx_recv_scan_chunk).  The 64-byte record is stored as four 16-byte quads by the
// first lanes of the group.  Selection (sx_recv_select) leaves one flag per row; a second kernel compacts the selected rows in row
// order with the workgroup scan of solo_wave.h -- a tile's base is the number of flags in front of it, which the tile counts itself, so no
// launch waits for another workgroup and the output is a pure function of the inputs.
//
// Counting (only with solo_recv_track on) is per stream, SX_RECV_TRK_WORDS words (solo_recv.h): the insert kernel adds the verdict
// of an arrival to its stream's counters, and a kernel of its own -- solo_recv_account_kernel, enqueued ahead of the play-out kernel --
// classifies the entries that are about to be played.  It is not part of solo_decode_ring_kernel because that kernel's registers and
// LDS are what the decoder's residency plan is built on.
//
// Everything outside the kernels compiles for the host as well (tests/test_recv_report_model.py builds sx_recv_report_host, which
// walks the rows group by group and chunk by chunk through the very functions of the kernels, and compares it with an independent model).
#pragma once
#include "solo_recv.h"
#include "solo_wave.h"          // wg_sum, wg_scan_incl
#include "solo_stream_ctl.h"

#define SX_RECV_TILE 256        // rows per workgroup of the compaction = its lanes (wg_sum / wg_scan_incl are for 256)

typedef solo_recv_report_t SxRecvReport;
static_assert(sizeof(SxRecvReport) == 64, "solo_recv_report_t layout");
typedef solo_recv_report_count_t SxRecvReportCount;
static_assert(sizeof(SxRecvReportCount) == 8, "solo_recv_report_count_t layout");

#define SX_RECV_REPORT_CLEAR_MARGIN SOLO_RECV_REPORT_CLEAR_MARGIN

// lanes that read one stream: the power of two at or above min(depth, 64)
SX_HD int sx_recv_group(int depth) {
    int g = 1;
    while (g < depth && g < 64) g <<= 1;
    return g;
}

// what a played packet was made of, from its entry's length word: 0 both descriptions, 1 MD1 only, 2 MD2 || HB only, 3 neither
SX_HD int sx_recv_play_class(u32 lw) {
    const int a = (lw & 0xFFFFu) != 0, b = (lw >> 16) != 0;
    return a ? (b ? 0 : 1) : (b ? 2 : 3);
}

// Scan of one stream's entries in physical order, up to 64 at a time.  r = p mod D is the entry of sequence number p.
//   f1 / l1: first empty / last filled entry at or above r (the front of the window);  f2 / l2: the same below r (its back)
struct SxRecvScan { i32 queued, complete, f1, f2, l1, l2, head; };
SX_HD void sx_recv_scan_init(SxRecvScan* s, int depth, int r) {
    s->queued = 0; s->complete = 0; s->f1 = depth; s->f2 = r; s->l1 = -1; s->l2 = -1; s->head = 0;
}
SX_HD int sx_recv_ctz64(u64 x) { return __builtin_ctzll(x); }
SX_HD int sx_recv_clz64(u64 x) { return __builtin_clzll(x); }
SX_HD int sx_recv_popc64(u64 x) { return __builtin_popcountll(x); }
// entries e0 .. e0 + cnt - 1 (1 <= cnt <= 64): bit k of mA / mB says whether slot A / B of entry e0 + k is filled
SX_HD void sx_recv_scan_chunk(SxRecvScan* s, u64 mA, u64 mB, int e0, int cnt, int r) {
    const u64 valid = cnt >= 64 ? ~(u64)0 : (((u64)1 << cnt) - 1);
    mA &= valid; mB &= valid;
    const u64 any = mA | mB, none = ~any & valid;
    const int cut = r - e0;                                  // bits at or above `cut` are entries >= r
    const u64 front = cut <= 0 ? valid : (cut >= 64 ? (u64)0 : (valid & (~(u64)0 << cut)));
    const u64 back = valid & ~front;
    s->queued += sx_recv_popc64(any);
    s->complete += sx_recv_popc64(mA & mB);
    if (none & front) s->f1 = sx_min(s->f1, e0 + sx_recv_ctz64(none & front));
    if (none & back) s->f2 = sx_min(s->f2, e0 + sx_recv_ctz64(none & back));
    if (any & front) s->l1 = sx_max(s->l1, e0 + 63 - sx_recv_clz64(any & front));
    if (any & back) s->l2 = sx_max(s->l2, e0 + 63 - sx_recv_clz64(any & back));
    if (cut >= 0 && cut < cnt) s->head = (i32)((mA >> cut) & 1) | ((i32)((mB >> cut) & 1) << 1);
}
struct SxRecvQueue { i32 play, queued, complete, ready, span, head; };
SX_HD SxRecvQueue sx_recv_scan_finish(const SxRecvScan* s, i32 play, int depth, int r) {
    SxRecvQueue q;
    q.play = play; q.queued = s->queued; q.complete = s->complete; q.head = s->head;
    q.ready = s->f1 < depth ? s->f1 - r : (depth - r) + s->f2;             // (the front is full: the run goes on at entry 0)
    q.span = s->l2 >= 0 ? s->l2 + depth - r + 1 : (s->l1 >= 0 ? s->l1 - r + 1 : 0);
    return q;
}

// the selection rule: enough packets in a row to start playing, or a queue about to overflow
SX_HD int sx_recv_select(i32 ready, i32 span, i32 m, i32 max_span) {
    return (m <= 0 || ready >= m) || (max_span > 0 && span >= max_span);
}

// word k (0 .. 15) of a stream's record; trk: the stream's counters, or NULL without them
SX_HD u32 sx_recv_report_word(int k, const SxRecvQueue& q, const u32* trk, int depth) {
    switch (k) {
        case 0: return (u32)q.play;
        case 1: return (u32)q.queued;
        case 2: return (u32)q.complete;
        case 3: return (u32)q.ready;
        case 4: return (u32)q.span;
        case 5: return (u32)q.head;
        case 15: return trk ? trk[SX_RECV_TRK_MARGIN] : (u32)depth;
        default: return trk ? trk[k - 6] : 0u;
    }
}

struct SxRecvReportArgs {
    const u32* lens; const i32* play; u32* trk; const i32* map; const i32* min_ready_v;
    u32* reports;               // [n][16] or NULL
    i32* sel;                   // [n]: 1 = the row is selected
    int n, depth, min_ready, max_span, clear_margin;
};

#if defined(__HIPCC__)
// 256 lanes = 4 wavefronts x (64 / G) rows; G = sx_recv_group(depth)
__global__ void __launch_bounds__(256) solo_recv_report_kernel(const SxRecvReportArgs a, int G, const u32* verdict) {
    if (sx_map_refused(a.map, verdict)) return;
    const int lane = (int)threadIdx.x & 63, j = lane & (G - 1), g0 = lane - j;
    const int row = ((int)blockIdx.x * 4 + ((int)threadIdx.x >> 6)) * (64 / G) + lane / G;
    const bool live = row < a.n;
    const int s = live ? (a.map ? a.map[row] : row) : 0;
    const i32 p = live ? a.play[s] : 0;
    const int r = (int)((u32)p % (u32)a.depth);
    const u32* l = a.lens + (size_t)s * (size_t)a.depth;
    SxRecvScan sc;
    sx_recv_scan_init(&sc, a.depth, r);
    for (int e0 = 0; e0 < a.depth; e0 += G) {               // (the trip count is the wavefront's: every lane takes part in the ballots)
        const int e = e0 + j;
        const u32 lw = (live && e < a.depth) ? l[e] : 0u;
        u64 mA = __ballot((lw & 0xFFFFu) != 0), mB = __ballot((lw >> 16) != 0);
        if (G < 64) { mA >>= g0; mB >>= g0; }
        sx_recv_scan_chunk(&sc, mA, mB, e0, sx_min(G, a.depth - e0), r);
    }
    if (!live) return;
    const SxRecvQueue q = sx_recv_scan_finish(&sc, p, a.depth, r);
    if (j == 0) a.sel[row] = sx_recv_select(q.ready, q.span, a.min_ready_v ? a.min_ready_v[row] : a.min_ready, a.max_span);
    u32* t = a.trk ? a.trk + (size_t)s * SX_RECV_TRK_WORDS : (u32*)0;
    if (a.reports)
        for (int qd = j; qd < 4; qd += G) {                 // one 16-byte quad per lane
            uint4 v;
            v.x = sx_recv_report_word(4 * qd + 0, q, t, a.depth); v.y = sx_recv_report_word(4 * qd + 1, q, t, a.depth);
            v.z = sx_recv_report_word(4 * qd + 2, q, t, a.depth); v.w = sx_recv_report_word(4 * qd + 3, q, t, a.depth);
            ((uint4*)a.reports)[(size_t)row * 4 + qd] = v;
        }
    // (the lane that read the margin is the one that sets it back: its own load and store stay in order)
    if (a.clear_margin && t && j == (3 & (G - 1))) t[SX_RECV_TRK_MARGIN] = (u32)a.depth;
}

// the selected rows, compacted in row order: list[k] = stream, rows[k] = row of the k-th selected row; count = {selected, n}
__global__ void __launch_bounds__(SX_RECV_TILE) solo_recv_compact_kernel(const i32* __restrict__ sel, const i32* __restrict__ map, int n, i32* __restrict__ list,
                                                                        i32* __restrict__ rows, SxRecvReportCount* count, const u32* verdict) {
    __shared__ i32 red[4], part[1][4];
    if (sx_map_refused(map, verdict)) {
        if (count && blockIdx.x == 0 && threadIdx.x == 0) count->selected = -1;
        return;
    }
    const int tid = (int)threadIdx.x, t0 = (int)blockIdx.x * SX_RECV_TILE;
    i32 before = 0;
    for (int i = tid; i < t0; i += SX_RECV_TILE) before += sel[i];
    before = wg_sum(before, red);
    const int i = t0 + tid;
    const i32 f = i < n ? sel[i] : 0;
    const i32 k = before + wg_scan_incl(f, part) - f;                         // (k < n: there are at most n flags)
    if (f) {
        if (list) list[k] = map ? map[i] : i;
        if (rows) rows[k] = i;
    }
    if (count && i == n - 1) { SxRecvReportCount c; c.selected = k + f; c.listed = n; *count = c; }
}

// Play-out accounting: one lane per played stream classifies the entries play .. play + n_packets - 1 that the play-out kernel behind
// it is going to decode and clear.  A stream is listed once, so its counters are this lane's alone.
__global__ void __launch_bounds__(256) solo_recv_account_kernel(const u32* __restrict__ lens, const i32* __restrict__ play, u32* trk, int n, int n_packets,
                                                                int depth, const i32* __restrict__ map, const u32* verdict) {
    if (sx_map_refused(map, verdict)) return;
    const int row = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (row >= n) return;
    const int s = map ? map[row] : row;
    const i32 p0 = play[s];
    u32 c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    for (int p = 0; p < n_packets; p++) {
        const int cls = sx_recv_play_class(lens[sx_recv_entry(s, p0 + p, depth)]);
        c0 += cls == 0; c1 += cls == 1; c2 += cls == 2; c3 += cls == 3;
    }
    u32* t = trk + (size_t)s * SX_RECV_TRK_WORDS + SX_RECV_TRK_PLAYED;
    t[0] += c0; t[1] += c1; t[2] += c2; t[3] += c3;
}

// counters of every stream / of the listed streams back to zero, margin_min to `depth` (= none)
__global__ void __launch_bounds__(256) solo_recv_trk_reset_kernel(u32* trk, int n_streams, int depth) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (size_t)n_streams * SX_RECV_TRK_WORDS) trk[i] = (i % SX_RECV_TRK_WORDS) == SX_RECV_TRK_MARGIN ? (u32)depth : 0u;
}
__global__ void __launch_bounds__(64) solo_recv_trk_reset_list_kernel(u32* trk, const SxStreamCtlList list, int n, int depth) {
    if ((int)blockIdx.x >= n) return;
    u32* t = trk + (size_t)list.r[blockIdx.x].stream * SX_RECV_TRK_WORDS;
    if (threadIdx.x < SX_RECV_TRK_WORDS) t[threadIdx.x] = threadIdx.x == SX_RECV_TRK_MARGIN ? (u32)depth : 0u;
}

static inline hipError_t solo_recv_report_launch(const SxRecvReportArgs& a, i32* list, i32* rows, SxRecvReportCount* count, const u32* verdict, hipStream_t s) {
    const int G = sx_recv_group(a.depth), rows_per_block = 4 * (64 / G);
    hipLaunchKernelGGL(solo_recv_report_kernel, dim3((unsigned)((a.n + rows_per_block - 1) / rows_per_block)), dim3(256), 0, s, a, G, verdict);
    if (list || rows || count)
        hipLaunchKernelGGL(solo_recv_compact_kernel, dim3((unsigned)((a.n + SX_RECV_TILE - 1) / SX_RECV_TILE)), dim3(SX_RECV_TILE), 0, s, a.sel, a.map, a.n, list,
                           rows, count, verdict);
    return hipGetLastError();
}
static inline hipError_t solo_recv_account_launch(const u32* lens, const i32* play, u32* trk, int n, int n_packets, int depth, const i32* map,
                                                  const u32* verdict, hipStream_t s) {
    hipLaunchKernelGGL(solo_recv_account_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, lens, play, trk, n, n_packets, depth, map, verdict);
    return hipGetLastError();
}
static inline hipError_t solo_recv_trk_reset_launch(u32* trk, int n_streams, int depth, hipStream_t s) {
    const size_t n = (size_t)n_streams * SX_RECV_TRK_WORDS;
    hipLaunchKernelGGL(solo_recv_trk_reset_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, trk, n_streams, depth);
    return hipGetLastError();
}
static inline hipError_t solo_recv_trk_reset_list_launch(u32* trk, const SxStreamCtl* recs, int n, int depth, hipStream_t s) {
    return sx_launch_ctl_batches(recs, n, [&](const SxStreamCtlList& l, int k) { hipLaunchKernelGGL(solo_recv_trk_reset_list_kernel, dim3(k), dim3(64), 0, s, trk, l, k, depth); });
}
#else
// Host form of the two kernels (tests): row by row, the group's lanes and chunks as in the kernel, through the functions above.
// Returns the number of selected rows; list / rows / reports may be NULL.
static inline int sx_recv_report_host(const SxRecvReportArgs& a, i32* list, i32* rows) {
    const int G = sx_recv_group(a.depth);
    int k = 0;
    for (int row = 0; row < a.n; row++) {
        const int s = a.map ? a.map[row] : row;
        const i32 p = a.play[s];
        const int r = (int)((u32)p % (u32)a.depth);
        const u32* l = a.lens + (size_t)s * (size_t)a.depth;
        SxRecvScan sc;
        sx_recv_scan_init(&sc, a.depth, r);
        for (int e0 = 0; e0 < a.depth; e0 += G) {
            u64 mA = 0, mB = 0;
            for (int j = 0; j < G; j++) {
                const u32 lw = e0 + j < a.depth ? l[e0 + j] : 0u;
                mA |= (u64)((lw & 0xFFFFu) != 0) << j; mB |= (u64)((lw >> 16) != 0) << j;
            }
            sx_recv_scan_chunk(&sc, mA, mB, e0, sx_min(G, a.depth - e0), r);
        }
        const SxRecvQueue q = sx_recv_scan_finish(&sc, p, a.depth, r);
        const int f = sx_recv_select(q.ready, q.span, a.min_ready_v ? a.min_ready_v[row] : a.min_ready, a.max_span);
        a.sel[row] = f;
        u32* t = a.trk ? a.trk + (size_t)s * SX_RECV_TRK_WORDS : (u32*)0;
        if (a.reports)
            for (int w = 0; w < 16; w++) a.reports[(size_t)row * 16 + w] = sx_recv_report_word(w, q, t, a.depth);
        if (a.clear_margin && t) t[SX_RECV_TRK_MARGIN] = (u32)a.depth;
        if (f) {
            if (list) list[k] = s;
            if (rows) rows[k] = row;
            k++;
        }
    }
    return k;
}
#endif

// solo_rtcp.h -- RTCP (RFC 3550 section 6.4) beside the RTP sessions of solo_rtp.h (solo_rtcp_received, solo_rtcp_sent, solo_rtcp_build,
// solo_rtcp_parse; include/solo_mi355x.h has the rules): reception statistics per stream from the arrivals solo_rtp_parse wrote, the
// sender's counts from the datagrams solo_rtp_pack left, compound SR / RR + SDES packets out of both, and the peers' compound packets
// into feedback records.  The sessions are read (their records and SSRC tables) and never written; the state lives here.
//
// A row (SxRtcpRow, 32 words; the object is a solo_rows of solo_api.hip, the CNAME its second segment of 8 words):
//      0 base_seq   1 max_seq   2 cycles   3 bad_seq   4 received   5 expected_prior   6 received_prior        RFC 3550 A.1 `source`
//      7 transit    8 jitter (x 16, A.8)   9 seen: 1 a datagram has counted | 2 transit is set | 4 an SR was parsed
//     10 lsr       11 lsr_arrival         12 tx_packets   13 tx_octets   14 tx_next   15 tx_since              16 .. 31 reserved, zero
// A zeroed row is a reset one: the first counting datagram runs init_seq.
//
// Received -- THE HOT PATH, every datagram passes here.  update_seq is sequential per stream, so the datagrams of a stream must pass
// in index order, whatever the interleaving:
//     1. begin    one lane: the counts and the list of flooding streams to zero
//     2. key      a lane per datagram: key[i] = its stream if it counts, else -1
//     3. - 6.     the room plan of solo_mix.h over the keys (clear, check = histogram, scan, scatter): members[starts[s] .. + counts[s])
//                 are the datagrams of stream s, in the order of the scatter's atomics
//     7. walk     ONE wavefront per stream with 1 .. SX_RTCP_WALK_MAX datagrams: every lane ranks its one or two indices among the
//                 segment's (LDS), the inputs {sequence number, transit} go to LDS in index order, lane 0 walks them with the row in
//                 registers.  A stream with more is appended to the list of flooding streams
//     8. flood    a workgroup per flooding stream (at most n_dgrams / (SX_RTCP_WALK_MAX + 1)): the keys tile by tile in index order, the
//                 tile's own datagrams compacted in order by the workgroup scan, lane 0 walks them
// Linear in the datagrams; a flooding stream costs one more pass over the keys and a serial walk of its own datagrams.
//
// Sent: a clear, then a lane per record with atomic add / max on the row.  Build: the list check of every device list, then the three
// passes of solo_rtp_pack (tile totals, one wavefront scans them, the tile again: a lane writes its packet, at most 96 bytes, and behind it
// the zeroed room solo_rtcp_set_trailer asked for: that of the SRTCP trailer, solo_srtcp.h).  Parse:
// a lane per datagram validates (A.2) and votes -- atomicMax of the datagram index per stream for SRs and for report blocks --, then the
// same walk again in which the winners write; a lane per row fills the feedback rows nobody won.
//
// Everything outside the kernels compiles for the host as well (tests/test_rtcp_model.py builds the host forms through
// tests/rtcp_host.cpp and compares them with the independent model of tests/rtcp_model.py).
#pragma once
#include "solo_rtp.h"
#include "solo_mix.h"

#define SX_RTCP_TILE 256
#define SX_RTCP_WORDS 32
#define SX_RTCP_CNAME_WORDS 8
#define SX_RTCP_WALK_MAX SOLO_RTCP_WALK_MAX
#define SX_RTCP_MAX_DROPOUT 3000u
#define SX_RTCP_MAX_MISORDER 100u
#define SX_RTCP_SEEN 1u
#define SX_RTCP_HAS_TRANSIT 2u
#define SX_RTCP_HAS_SR 4u

struct SxRtcpRow {
    u32 base_seq, max_seq, cycles, bad_seq, received, expected_prior, received_prior, transit, jitter, seen, lsr, lsr_arrival;
    u32 tx_packets, tx_octets, tx_next, tx_since, reserved[16];
};
static_assert(sizeof(SxRtcpRow) == SOLO_RTCP_STATE_BYTES && SOLO_RTCP_STATE_BYTES == 4 * SX_RTCP_WORDS, "a row of the state");
static_assert(SOLO_RTCP_CNAME_BYTES == 4 * SX_RTCP_CNAME_WORDS, "the CNAME segment");
typedef solo_rtcp_received_count_t SxRtcpRecvCount;
static_assert(sizeof(SxRtcpRecvCount) == 32, "solo_rtcp_received_count_t layout");
typedef solo_rtcp_sent_count_t SxRtcpSentCount;
static_assert(sizeof(SxRtcpSentCount) == 32, "solo_rtcp_sent_count_t layout");
typedef solo_rtcp_build_count_t SxRtcpBuildCount;
static_assert(sizeof(SxRtcpBuildCount) == 32, "solo_rtcp_build_count_t layout");
typedef solo_rtcp_parse_count_t SxRtcpParseCount;
static_assert(sizeof(SxRtcpParseCount) == 64, "solo_rtcp_parse_count_t layout");
typedef solo_rtcp_feedback_t SxRtcpFeedback;
static_assert(sizeof(SxRtcpFeedback) == 32, "solo_rtcp_feedback_t layout");

// the read-modify-write steps of the lane-per-item passes: atomics on the device, plain in the 1-lane host form
SX_HD void sx_rtcp_add(u32* p, u32 v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(p, v);
#else
    *p += v;
#endif
}
SX_HD void sx_rtcp_add(i32* p, i32 v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(p, v);
#else
    *p += v;
#endif
}
SX_HD void sx_rtcp_max(u32* p, u32 v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMax(p, v);
#else
    if (v > *p) *p = v;
#endif
}
SX_HD void sx_rtcp_max(i32* p, i32 v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMax(p, v);
#else
    if (v > *p) *p = v;
#endif
}
SX_HD void sx_rtcp_or(i32* p, i32 v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicOr(p, v);
#else
    *p |= v;
#endif
}
SX_HD u32 sx_rtcp_mid32(unsigned long long ntp) { return (u32)(ntp >> 16); }

// what the object keeps per stream beside the rows, sized at create (words): counts | starts | cursor of the room plan, the flooding
// streams {number, streams ...}, parse's four vote arrays, build's tile totals {valid, refused, bytes} and tile bases (64 bits)
static inline size_t solo_rtcp_plan_words(int n_streams) {
    const size_t n = (size_t)n_streams, tiles = (n + SX_RTCP_TILE - 1) / SX_RTCP_TILE;
    return 2 * tiles + 3 * n + (n + 1) + 4 * n + 3 * tiles + 1;
}
struct SxRtcpPlanMem { i64* bases; i32* counts; i32* starts; i32* cursor; i32* big; i32* win; i32* totals; };
static inline SxRtcpPlanMem sx_rtcp_plan_mem(void* at, int n_streams) {
    const size_t n = (size_t)n_streams, tiles = (n + SX_RTCP_TILE - 1) / SX_RTCP_TILE;
    SxRtcpPlanMem m;
    m.bases = (i64*)at; m.counts = (i32*)(m.bases + tiles); m.starts = m.counts + n; m.cursor = m.starts + n; m.big = m.cursor + n;
    m.win = m.big + n + 1; m.totals = m.win + 4 * n;
    return m;
}
// ... and per datagram of a call (bytes): received's key | members, parse's verdicts
static inline size_t solo_rtcp_scratch_bytes(int n_dgrams) { return 2 * (size_t)n_dgrams * sizeof(i32) + 16; }

// ---- the control plane ---------------------------------------------------------------------------------------------------------------
// names [n][32]: every one 1 .. 31 bytes and NUL-padded from its end to byte 31
static inline bool sx_rtcp_cname_ok(const int32_t* streams, int32_t n, const char* names, int32_t n_streams) {
    if (!names || !sx_list_ok(streams, n, n_streams)) return false;
    for (int32_t i = 0; i < n; i++) {
        const char* c = names + (size_t)i * SOLO_RTCP_CNAME_BYTES;
        if (c[0] == 0) return false;
        int len = 0;
        while (len < SOLO_RTCP_CNAME_BYTES && c[len] != 0) len++;
        if (len >= SOLO_RTCP_CNAME_BYTES) return false;
        for (int k = len; k < SOLO_RTCP_CNAME_BYTES; k++)
            if (c[k] != 0) return false;
    }
    return true;
}

// ---- received --------------------------------------------------------------------------------------------------------------------------
#define SX_RTCP_C_COUNTED 0
#define SX_RTCP_C_FIRST 1
#define SX_RTCP_C_IN_ORDER 2
#define SX_RTCP_C_MISORDERED 3
#define SX_RTCP_C_DROPOUT 4
#define SX_RTCP_C_RESYNCED 5
#define SX_RTCP_C_NOT_COUNTED 6

struct SxRtcpRecvArgs {
    const SxSendRecord* arrivals; const uint16_t* rtp_seq; const u32* arrival_time;     // [n_dgrams]; arrival_time NULL: now_rtp
    const SxRtpStream* cfg; SxRtcpRow* state;                                            // [n_streams]
    i32* key; i32* members;                                                              // [n_dgrams] of the scratch
    i32* counts; i32* starts; i32* cursor; i32* big;                                     // the object's (SxRtcpPlanMem)
    i32* count;                                                                          // SxRtcpRecvCount
    u32 now_rtp;
    int n_dgrams, n_streams, packet_samples;
};
static inline bool sx_rtcp_received_ok(const void* c, int n_streams, int session_streams, const void* arrivals, const void* rtp_seq, int n_dgrams,
                                       const void* arrival_time, const void* count) {
    if (!c || !count || session_streams != n_streams || n_dgrams < 0 || (n_dgrams > 0 && (!arrivals || !rtp_seq))) return false;
    return !(((uintptr_t)arrivals | (uintptr_t)arrival_time | (uintptr_t)count) & 3) && !((uintptr_t)rtp_seq & 1);
}
SX_HD void sx_rtcp_init_seq(SxRtcpRow& s, u32 seq) {
    s.base_seq = seq; s.max_seq = seq; s.bad_seq = 65537u; s.cycles = 0; s.received = 0; s.received_prior = 0; s.expected_prior = 0;
}
// THE datagram rule: sequence number `seq` (16 bits) with transit time `transit` -> the row, and the counter of its outcome
SX_HD int sx_rtcp_update(SxRtcpRow& s, u32 seq, u32 transit) {
    int out;
    if (!(s.seen & SX_RTCP_SEEN)) {
        sx_rtcp_init_seq(s, seq);
        s.seen |= SX_RTCP_SEEN;
        out = SX_RTCP_C_FIRST;
    } else {
        const u32 udelta = (seq - s.max_seq) & 0xFFFFu;
        if (udelta < SX_RTCP_MAX_DROPOUT) {
            if (seq < s.max_seq) s.cycles += 65536u;
            s.max_seq = seq;
            out = SX_RTCP_C_IN_ORDER;
        } else if (udelta <= 65536u - SX_RTCP_MAX_MISORDER) {
            if (seq != s.bad_seq) {
                s.bad_seq = (seq + 1u) & 0xFFFFu;
                return SX_RTCP_C_DROPOUT;
            }
            sx_rtcp_init_seq(s, seq);
            out = SX_RTCP_C_RESYNCED;
        } else {
            out = SX_RTCP_C_MISORDERED;
        }
    }
    s.received++;
    if (s.seen & SX_RTCP_HAS_TRANSIT) {
        const i32 d = (i32)(transit - s.transit);
        const u32 ad = d < 0 ? 0u - (u32)d : (u32)d;
        s.jitter += ad - ((s.jitter + 8u) >> 4);
    }
    s.transit = transit;
    s.seen |= SX_RTCP_HAS_TRANSIT;
    return out;
}
SX_HD i32 sx_rtcp_key(const SxRtcpRecvArgs& a, int i) {
    const i32 s = a.arrivals[i].stream;
    return (s >= 0 && s < a.n_streams) ? s : -1;
}
// the two inputs of datagram i of stream s
SX_HD void sx_rtcp_inputs(const SxRtcpRecvArgs& a, int s, int i, u32* in) {
    in[0] = (u32)a.rtp_seq[i];
    in[1] = (a.arrival_time ? a.arrival_time[i] : a.now_rtp) - (a.cfg[s].ts_offset + (u32)a.arrivals[i].seq * (u32)a.packet_samples);
}
// One stream with 1 .. SX_RTCP_WALK_MAX datagrams: what one wavefront does.  seg [SX_RTCP_WALK_MAX], in [2 SX_RTCP_WALK_MAX]: LDS;
// cnt [8]: lane 0 adds the outcomes.  -> true: the stream has more, nothing was done
SX_HD bool sx_rtcp_walk_small(const SxRtcpRecvArgs& a, int s, i32* seg, u32* in, i32* cnt) {
    const int c = SX_UNI(a.counts[s]), first = SX_UNI(a.starts[s]);
    if (c <= 0) return false;
    if (c > SX_RTCP_WALK_MAX) return true;
    SX_PAR(j, c) seg[j] = a.members[first + j];
    wv_sync();
    SX_PAR(j, c) {
        const i32 x = seg[j];
        int rk = 0;
        for (int t = 0; t < c; t++) rk += seg[t] < x;
        sx_rtcp_inputs(a, s, x, in + 2 * rk);
    }
    wv_sync();
    if (SX_LANE == 0) {
        SxRtcpRow row = a.state[s];
        for (int j = 0; j < c; j++) cnt[sx_rtcp_update(row, in[2 * j], in[2 * j + 1])]++;
        a.state[s] = row;
    }
    return false;
}

#if defined(__HIPCC__)
__global__ void __launch_bounds__(64) solo_rtcp_received_begin_kernel(const SxRtcpRecvArgs a) {
    if (threadIdx.x < 8) a.count[threadIdx.x] = 0;
    if (threadIdx.x == 8) a.big[0] = 0;
}
__global__ void __launch_bounds__(SX_RTCP_TILE) solo_rtcp_key_kernel(const SxRtcpRecvArgs a) {
    __shared__ i32 red[4];
    const int i = (int)blockIdx.x * SX_RTCP_TILE + (int)threadIdx.x;
    i32 k = 0;
    if (i < a.n_dgrams) {
        k = sx_rtcp_key(a, i);
        a.key[i] = k;
    }
    const i32 out = wg_sum(k < 0 ? 1 : 0, red);
    if (threadIdx.x == 0 && out) atomicAdd(&a.count[SX_RTCP_C_NOT_COUNTED], out);
}
__global__ void __launch_bounds__(64) solo_rtcp_walk_kernel(const SxRtcpRecvArgs a) {
    __shared__ i32 seg[SX_RTCP_WALK_MAX];
    __shared__ u32 in[2 * SX_RTCP_WALK_MAX];
    __shared__ i32 cnt[8];
    const int s = (int)blockIdx.x;
    if (threadIdx.x < 8) cnt[threadIdx.x] = 0;
    __syncthreads();
    const bool more = sx_rtcp_walk_small(a, s, seg, in, cnt);
    __syncthreads();
    if (more) {
        if (threadIdx.x == 0) a.big[1 + atomicAdd(&a.big[0], 1)] = s;
        return;
    }
    const int t = (int)threadIdx.x;
    if (t >= 1 && t < 6 && cnt[t]) { atomicAdd(&a.count[t], cnt[t]); atomicAdd(&a.count[SX_RTCP_C_COUNTED], cnt[t]); }
}
// a workgroup per flooding stream: the keys in index order, SX_RTCP_TILE at a time
__global__ void __launch_bounds__(SX_RTCP_TILE) solo_rtcp_flood_kernel(const SxRtcpRecvArgs a) {
    __shared__ i32 part[1][4];
    __shared__ u32 in[2 * SX_RTCP_TILE];
    __shared__ i32 cnt[8];
    if ((i32)blockIdx.x >= a.big[0]) return;
    const int s = a.big[1 + blockIdx.x], tid = (int)threadIdx.x;
    if (tid < 8) cnt[tid] = 0;
    SxRtcpRow row;
    if (tid == 0) row = a.state[s];
    __syncthreads();
    for (int i0 = 0; i0 < a.n_dgrams; i0 += SX_RTCP_TILE) {
        const int i = i0 + tid;
        const bool mine = i < a.n_dgrams && a.key[i] == s;
        const i32 incl = wg_scan_incl(mine ? 1 : 0, part);
        if (mine) sx_rtcp_inputs(a, s, i, in + 2 * (incl - 1));
        __syncthreads();
        if (tid == 0) {
            const i32 m = wg_total(part[0]);
            for (int j = 0; j < m; j++) cnt[sx_rtcp_update(row, in[2 * j], in[2 * j + 1])]++;
        }
        __syncthreads();            // (in[] and part[] are the next tile's as well)
    }
    if (tid == 0) a.state[s] = row;
    if (tid >= 1 && tid < 6 && cnt[tid]) { atomicAdd(&a.count[tid], cnt[tid]); atomicAdd(&a.count[SX_RTCP_C_COUNTED], cnt[tid]); }
}
// a.key / a.members: the scratch; a.counts .. a.big: the object's; verdict: the plan's word (the keys are all inside [-1, n_streams): it stays 0)
static inline hipError_t solo_rtcp_received_launch(const SxRtcpRecvArgs& a, u32* verdict, hipStream_t s) {
    hipLaunchKernelGGL(solo_rtcp_received_begin_kernel, dim3(1), dim3(64), 0, s, a);
    if (a.n_dgrams == 0) return hipGetLastError();
    hipLaunchKernelGGL(solo_rtcp_key_kernel, dim3((unsigned)((a.n_dgrams + SX_RTCP_TILE - 1) / SX_RTCP_TILE)), dim3(SX_RTCP_TILE), 0, s, a);
    SxRoomPlan rp;
    rp.counts = a.counts; rp.starts = a.starts; rp.cursor = a.cursor; rp.members = a.members;
    sx_room_plan_launch(rp, a.key, a.n_dgrams, a.n_streams, NULL, verdict, [](u32*) {}, s);
    hipLaunchKernelGGL(solo_rtcp_walk_kernel, dim3((unsigned)a.n_streams), dim3(64), 0, s, a);
    const int most = a.n_dgrams / (SX_RTCP_WALK_MAX + 1);
    if (most > 0) hipLaunchKernelGGL(solo_rtcp_flood_kernel, dim3((unsigned)sx_min(most, a.n_streams)), dim3(SX_RTCP_TILE), 0, s, a);
    return hipGetLastError();
}
#else
// Host form (tests): the same passes; the plan's lists come filled from the LAST datagram down, so the ranking has work to do
static inline void sx_rtcp_received_host(SxRtcpRecvArgs a) {
    std::vector<i32> key((size_t)a.n_dgrams + 1), members((size_t)a.n_dgrams + 1), plan(3 * (size_t)a.n_streams, 0), seg(SX_RTCP_WALK_MAX);
    std::vector<u32> in(2 * SX_RTCP_WALK_MAX);
    i32 cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    a.key = key.data(); a.members = members.data(); a.counts = plan.data(); a.starts = a.counts + a.n_streams; a.cursor = a.starts + a.n_streams;
    for (int i = 0; i < a.n_dgrams; i++) {
        key[i] = sx_rtcp_key(a, i);
        cnt[SX_RTCP_C_NOT_COUNTED] += key[i] < 0;
    }
    SxRoomPlan rp;
    rp.counts = a.counts; rp.starts = a.starts; rp.cursor = a.cursor; rp.members = a.members;
    i32 rows, rooms;
    sx_room_plan_host(rp, a.key, a.n_dgrams, a.n_streams, &rows, &rooms);
    for (int s = 0; s < a.n_streams; s++) {
        if (!sx_rtcp_walk_small(a, s, seg.data(), in.data(), cnt)) continue;
        SxRtcpRow row = a.state[s];                          // the flood: the keys in index order
        for (int i = 0; i < a.n_dgrams; i++)
            if (key[i] == s) {
                u32 x[2];
                sx_rtcp_inputs(a, s, i, x);
                cnt[sx_rtcp_update(row, x[0], x[1])]++;
            }
        a.state[s] = row;
    }
    for (int t = 1; t < 6; t++) cnt[SX_RTCP_C_COUNTED] += cnt[t];
    memcpy(a.count, cnt, 8 * sizeof(i32));
}
#endif

// ---- sent ------------------------------------------------------------------------------------------------------------------------------
struct SxRtcpSentArgs {
    const SxSendRecord* records; const SxSendCount* send_count; const SxRtpDgram* dgrams; SxRtcpRow* state; i32* count;
    int max_records, n_streams;
};
static inline bool sx_rtcp_sent_ok(const void* c, int n_streams, int session_streams, const void* records, const void* send_count, int max_records,
                                   const void* dgrams, const void* count) {
    if (!c || !records || !send_count || !dgrams || !count || session_streams != n_streams || max_records <= 0) return false;
    return !(((uintptr_t)records | (uintptr_t)send_count | (uintptr_t)dgrams | (uintptr_t)count) & 3);
}
SX_HD i32 sx_rtcp_sent_n(const SxRtcpSentArgs& a) { return sx_min(a.send_count->records, a.max_records); }
// THE record rule -> sent
SX_HD bool sx_rtcp_sent_one(const SxRtcpSentArgs& a, int k) {
    const SxSendRecord r = a.records[k];
    if (a.dgrams[k].len <= 0 || r.stream < 0 || r.stream >= a.n_streams) return false;
    SxRtcpRow* s = &a.state[r.stream];
    sx_rtcp_add(&s->tx_packets, 1u);
    sx_rtcp_add(&s->tx_octets, (u32)r.len);
    sx_rtcp_add(&s->tx_since, 1u);
    sx_rtcp_max(&s->tx_next, (u32)r.seq + 1u);
    return true;
}
#if defined(__HIPCC__)
__global__ void __launch_bounds__(64) solo_rtcp_sent_begin_kernel(const SxRtcpSentArgs a) {
    if (threadIdx.x < 8) a.count[threadIdx.x] = (threadIdx.x == 0 && sx_rtcp_sent_n(a) < 0) ? -1 : 0;
}
__global__ void __launch_bounds__(SX_RTCP_TILE) solo_rtcp_sent_kernel(const SxRtcpSentArgs a) {
    __shared__ i32 red[4];
    const i32 n = sx_rtcp_sent_n(a);
    if (n < 0 || (i32)blockIdx.x * SX_RTCP_TILE >= n) return;
    const int k = (int)blockIdx.x * SX_RTCP_TILE + (int)threadIdx.x;
    i32 sent = 0, skipped = 0;
    if (k < n) {
        sent = sx_rtcp_sent_one(a, k) ? 1 : 0;
        skipped = 1 - sent;
    }
    sent = wg_sum(sent, red);
    skipped = wg_sum(skipped, red);
    if (threadIdx.x == 0) {
        if (sent) atomicAdd(&a.count[0], sent);
        if (skipped) atomicAdd(&a.count[1], skipped);
    }
}
static inline hipError_t solo_rtcp_sent_launch(const SxRtcpSentArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(solo_rtcp_sent_begin_kernel, dim3(1), dim3(64), 0, s, a);
    hipLaunchKernelGGL(solo_rtcp_sent_kernel, dim3((unsigned)((a.max_records + SX_RTCP_TILE - 1) / SX_RTCP_TILE)), dim3(SX_RTCP_TILE), 0, s, a);
    return hipGetLastError();
}
#else
static inline void sx_rtcp_sent_host(const SxRtcpSentArgs& a) {
    const i32 n = sx_rtcp_sent_n(a);
    for (int w = 0; w < 8; w++) a.count[w] = 0;
    if (n < 0) { a.count[0] = -1; return; }
    for (int k = 0; k < n; k++) a.count[sx_rtcp_sent_one(a, k) ? 0 : 1]++;
}
#endif

// ---- build -----------------------------------------------------------------------------------------------------------------------------
struct SxRtcpBuildArgs {
    const i32* streams; const SxRtpStream* cfg_tx; const SxRtpStream* cfg_rx;            // cfg_rx NULL: no report blocks
    SxRtcpRow* state; const u32* cname;                                                  // [n_streams], [n_streams][8]
    const unsigned long long* d_now; unsigned long long now;                            // d_now NULL: the scalar
    SxRtpDgram* dgrams; u8* wire; i64 cap; SxRtcpBuildCount* count;
    i32* totals; i64* bases;                                                             // [tiles][3], [tiles]: the object's
    int n, n_streams, packet_samples;
    int trailer = 0;                                        // bytes kept free behind every packet (solo_rtcp_set_trailer: the SRTCP trailer's room), written as zero
};
static inline bool sx_rtcp_build_ok(const void* c, int n_streams, int tx_streams, bool has_rx, int rx_streams, const void* streams, int n, const void* d_now,
                                    const void* dgrams, const void* wire, long long cap, const void* count) {
    if (!c || !streams || !dgrams || !wire || !count || tx_streams != n_streams || (has_rx && rx_streams != n_streams)) return false;
    if (n <= 0 || n > n_streams || cap < 0) return false;
    return !(((uintptr_t)streams | (uintptr_t)dgrams | (uintptr_t)wire) & 3) && !(((uintptr_t)d_now | (uintptr_t)count) & 7);
}
struct SxRtcpPlan { i32 len, sr, rb, name_len; };            // bytes of the compound packet (0: refused), SR or RR, report blocks, bytes of the CNAME
SX_HD int sx_rtcp_name_len(const u32* name) {
    const u8* c = (const u8*)name;
    int len = 0;
    while (len < SOLO_RTCP_CNAME_BYTES - 1 && c[len] != 0) len++;
    return len;
}
SX_HD i32 sx_rtcp_sdes_bytes(int name_len) { return sx_rtp_roundup4(4 + 4 + 2 + name_len + 1); }
// THE packet rule, first half: listed stream i -> what its packet holds
SX_HD SxRtcpPlan sx_rtcp_build_plan(const SxRtcpBuildArgs& a, int i) {
    SxRtcpPlan p; p.len = 0; p.sr = 0; p.rb = 0; p.name_len = 0;
    const i32 s = a.streams[i];
    if (s < 0 || s >= a.n_streams || !a.cfg_tx[s].bound) return p;
    p.name_len = sx_rtcp_name_len(a.cname + (size_t)s * SX_RTCP_CNAME_WORDS);
    if (p.name_len == 0) return p;
    const SxRtcpRow& r = a.state[s];
    p.sr = r.tx_since > 0;
    p.rb = a.cfg_rx && a.cfg_rx[s].bound && (r.seen & SX_RTCP_SEEN);
    p.len = (p.sr ? 28 : 8) + 24 * p.rb + sx_rtcp_sdes_bytes(p.name_len);
    return p;
}
// what a packet of len bytes takes of the wire: itself, the trailer and the pad bytes up to a multiple of 4 (0 for a refused stream)
SX_HD i32 sx_rtcp_padded(const SxRtcpBuildArgs& a, i32 len) { return len > 0 ? sx_rtp_roundup4(len + a.trailer) : 0; }
SX_HD unsigned long long sx_rtcp_now(const unsigned long long* d_now, unsigned long long now) { return d_now ? *d_now : now; }
// ... second half: the bytes at dst (4-byte aligned), and the row's state behind a written packet
SX_HD void sx_rtcp_build_write(const SxRtcpBuildArgs& a, int i, const SxRtcpPlan& p, u8* dst) {
    const i32 s = a.streams[i];
    SxRtcpRow& r = a.state[s];
    const unsigned long long now = sx_rtcp_now(a.d_now, a.now);
    const u32 ssrc = a.cfg_tx[s].ssrc;
    u32* d = (u32*)dst;
    int w = 0;
    const u32 words = (u32)((p.sr ? 28 : 8) + 24 * p.rb) / 4u;
    d[w++] = sx_rtp_bswap(0x80000000u | ((u32)p.rb << 24) | ((p.sr ? 200u : 201u) << 16) | (words - 1u));
    d[w++] = sx_rtp_bswap(ssrc);
    if (p.sr) {
        d[w++] = sx_rtp_bswap((u32)(now >> 32));
        d[w++] = sx_rtp_bswap((u32)now);
        d[w++] = sx_rtp_bswap(a.cfg_tx[s].ts_offset + r.tx_next * (u32)a.packet_samples);
        d[w++] = sx_rtp_bswap(r.tx_packets);
        d[w++] = sx_rtp_bswap(r.tx_octets);
    }
    if (p.rb) {
        const u32 expected = r.cycles + r.max_seq - r.base_seq + 1u;
        i32 lost = (i32)(expected - r.received);
        lost = lost > 0x7FFFFF ? 0x7FFFFF : (lost < -0x800000 ? -0x800000 : lost);
        const u32 expected_interval = expected - r.expected_prior;
        const i32 lost_interval = (i32)(expected_interval - (r.received - r.received_prior));
        u32 fraction = 0;
        if (expected_interval != 0 && lost_interval > 0) {
            const unsigned long long f = ((unsigned long long)(u32)lost_interval << 8) / expected_interval;
            fraction = f > 255 ? 255u : (u32)f;
        }
        d[w++] = sx_rtp_bswap(a.cfg_rx[s].ssrc);
        d[w++] = sx_rtp_bswap((fraction << 24) | ((u32)lost & 0xFFFFFFu));
        d[w++] = sx_rtp_bswap(r.cycles | r.max_seq);
        d[w++] = sx_rtp_bswap(r.jitter >> 4);
        d[w++] = sx_rtp_bswap((r.seen & SX_RTCP_HAS_SR) ? r.lsr : 0u);
        d[w++] = sx_rtp_bswap((r.seen & SX_RTCP_HAS_SR) ? sx_rtcp_mid32(now) - r.lsr_arrival : 0u);
        r.expected_prior = expected; r.received_prior = r.received;
    }
    const i32 sdes = sx_rtcp_sdes_bytes(p.name_len);
    d[w++] = sx_rtp_bswap(0x81000000u | (202u << 16) | (u32)(sdes / 4 - 1));
    d[w++] = sx_rtp_bswap(ssrc);
    u8* b = (u8*)(d + w);
    const u8* name = (const u8*)(a.cname + (size_t)s * SX_RTCP_CNAME_WORDS);
    b[0] = 1; b[1] = (u8)p.name_len;
    for (int k = 0; k < p.name_len; k++) b[2 + k] = name[k];
    for (int k = 2 + p.name_len; k < sdes - 8; k++) b[k] = 0;
    for (int k = p.len / 4; k < sx_rtcp_padded(a, p.len) / 4; k++) d[k] = 0;     // (the trailer and its pad: whole dwords, none without a trailer)
    r.tx_since = 0;
}
#if defined(__HIPCC__)
__global__ void __launch_bounds__(SX_RTCP_TILE) solo_rtcp_build_totals_kernel(const SxRtcpBuildArgs a, const u32* verdict) {
    __shared__ i32 red[4];
    if (sx_map_refused(a.streams, verdict)) return;
    const int i = (int)blockIdx.x * SX_RTCP_TILE + (int)threadIdx.x;
    i32 len = 0, listed = 0;
    if (i < a.n) { len = sx_rtcp_build_plan(a, i).len; listed = 1; }
    const i32 valid = wg_sum(len > 0 ? 1 : 0, red), refused = wg_sum(listed && len == 0 ? 1 : 0, red), bytes = wg_sum(sx_rtcp_padded(a, len), red);
    if (threadIdx.x == 0) { a.totals[blockIdx.x * 3 + 0] = valid; a.totals[blockIdx.x * 3 + 1] = refused; a.totals[blockIdx.x * 3 + 2] = bytes; }
}
__global__ void __launch_bounds__(64) solo_rtcp_build_scan_kernel(const SxRtcpBuildArgs a, int n_tiles, const u32* verdict) {
    if (sx_map_refused(a.streams, verdict)) {
        if (threadIdx.x == 0) a.count->built = -1;
        return;
    }
    i64 base = 0;
    i32 valid = 0, refused = 0;
    for (int t0 = 0; t0 < n_tiles; t0 += 64) {
        const int t = t0 + (int)threadIdx.x;
        const i32 bytes = t < n_tiles ? a.totals[t * 3 + 2] : 0;
        const i32 incl = wv_scan_incl(bytes);
        if (t < n_tiles) a.bases[t] = base + (i64)(incl - bytes);
        base += (i64)__builtin_amdgcn_readlane(incl, 63);
        valid += wv_sum(t < n_tiles ? a.totals[t * 3 + 0] : 0);
        refused += wv_sum(t < n_tiles ? a.totals[t * 3 + 1] : 0);
    }
    if (threadIdx.x == 0) {
        SxRtcpBuildCount c; c.built = 0; c.built_needed = valid; c.bytes = 0; c.bytes_needed = base; c.refused = refused; c.with_sr = 0;
        *a.count = c;
    }
}
__global__ void __launch_bounds__(SX_RTCP_TILE) solo_rtcp_build_kernel(const SxRtcpBuildArgs a, const u32* verdict) {
    __shared__ i32 red[4], part[1][4];
    if (sx_map_refused(a.streams, verdict)) return;
    const int i = (int)blockIdx.x * SX_RTCP_TILE + (int)threadIdx.x;
    SxRtcpPlan p; p.len = 0; p.sr = 0; p.rb = 0; p.name_len = 0;
    if (i < a.n) p = sx_rtcp_build_plan(a, i);
    const i32 padded = sx_rtcp_padded(a, p.len);
    const i32 incl = wg_scan_incl(padded, part);
    bool written = false;
    if (i < a.n) {
        const i64 off = a.bases[blockIdx.x] + (i64)(incl - padded);
        written = sx_rtp_pack_emit(a.dgrams, i, p.len, padded, off, a.cap);
        if (written) sx_rtcp_build_write(a, i, p, a.wire + off);
    }
    const i32 n_written = wg_sum(written ? 1 : 0, red), n_sr = wg_sum(written && p.sr ? 1 : 0, red), bytes = wg_sum(written ? padded : 0, red);
    if (threadIdx.x == 0 && n_written) {
        atomicAdd(&a.count->built, n_written);
        if (n_sr) atomicAdd(&a.count->with_sr, n_sr);
        atomicAdd((unsigned long long*)&a.count->bytes, (unsigned long long)bytes);
    }
}
// verdict: the word the list check of a.streams has written (the caller enqueues it in front)
static inline hipError_t solo_rtcp_build_launch(SxRtcpBuildArgs a, const u32* verdict, hipStream_t s) {
    const int n_tiles = (a.n + SX_RTCP_TILE - 1) / SX_RTCP_TILE;
    if (a.cap > 0x7FFFFFFFLL) a.cap = 0x7FFFFFFFLL;
    hipLaunchKernelGGL(solo_rtcp_build_totals_kernel, dim3((unsigned)n_tiles), dim3(SX_RTCP_TILE), 0, s, a, verdict);
    hipLaunchKernelGGL(solo_rtcp_build_scan_kernel, dim3(1), dim3(64), 0, s, a, n_tiles, verdict);
    hipLaunchKernelGGL(solo_rtcp_build_kernel, dim3((unsigned)n_tiles), dim3(SX_RTCP_TILE), 0, s, a, verdict);
    return hipGetLastError();
}
#else
// -> false: the list was refused, built = -1 and nothing else written
static inline bool sx_rtcp_build_host(SxRtcpBuildArgs a) {
    if (!sx_map_ok(a.streams, a.n, a.n_streams)) { a.count->built = -1; return false; }
    if (a.cap > 0x7FFFFFFFLL) a.cap = 0x7FFFFFFFLL;
    SxRtcpBuildCount c; c.built = 0; c.built_needed = 0; c.bytes = 0; c.bytes_needed = 0; c.refused = 0; c.with_sr = 0;
    std::vector<SxRtcpPlan> plans((size_t)a.n);
    for (int i = 0; i < a.n; i++) {                          // (all plans first: they read the state the writes change)
        plans[i] = sx_rtcp_build_plan(a, i);
        if (plans[i].len > 0) c.built_needed++;
        else c.refused++;
    }
    for (int i = 0; i < a.n; i++) {
        const SxRtcpPlan& p = plans[i];
        const i32 padded = sx_rtcp_padded(a, p.len);
        if (sx_rtp_pack_emit(a.dgrams, i, p.len, padded, c.bytes_needed, a.cap)) {
            sx_rtcp_build_write(a, i, p, a.wire + c.bytes_needed);
            c.built++; c.bytes += padded; c.with_sr += p.sr;
        }
        c.bytes_needed += padded;
    }
    *a.count = c;
    return true;
}
#endif

// ---- parse -----------------------------------------------------------------------------------------------------------------------------
#define SX_RTCP_ACCEPTED 0
#define SX_RTCP_MALFORMED 1
#define SX_RTCP_VERSION 2
#define SX_RTCP_FIRST_TYPE 3
#define SX_RTCP_LENGTH 4
#define SX_RTCP_P_SR 5              // (words of SxRtcpParseCount behind the verdicts)
#define SX_RTCP_P_BLOCKS 6
#define SX_RTCP_P_UNKNOWN 7
#define SX_RTCP_P_BYE 8
#define SX_RTCP_P_SKIPPED 9
#define SX_RTCP_P_WORDS 16

struct SxRtcpParseArgs {
    const SxRtpDgram* dgrams; const u8* wire; const u32* table_rx; const u32* table_tx;   // table_tx NULL: no feedback
    SxRtcpRow* state; i32* win;                                                           // win [4][n_streams]: SR winner, block winner, blocks, bye
    i32* ok;                                                                              // [n_dgrams] of the scratch: the verdicts
    SxRtcpFeedback* feedback; i32* count;
    const unsigned long long* d_now; unsigned long long now;
    i64 wire_bytes;
    int n_dgrams, n_streams;
};
static inline bool sx_rtcp_parse_ok(const void* c, int n_streams, int rx_streams, bool has_tx, int tx_streams, const void* dgrams, int n_dgrams, const void* wire,
                                    long long wire_bytes, const void* d_now, const void* feedback, const void* count) {
    if (!c || !feedback || !count || rx_streams != n_streams || (has_tx && tx_streams != n_streams)) return false;
    if (n_dgrams < 0 || wire_bytes < 0 || (n_dgrams > 0 && (!dgrams || !wire))) return false;
    return !(((uintptr_t)dgrams | (uintptr_t)feedback) & 3) && !(((uintptr_t)d_now | (uintptr_t)count) & 7);
}
// bytes behind the header that a packet of type pt with count rc announces
SX_HD i32 sx_rtcp_body_needed(u32 pt, u32 rc) { return pt == 200u ? 24 + 24 * (i32)rc : pt == 201u ? 4 + 24 * (i32)rc : pt == 203u ? 4 * (i32)rc : 0; }
// THE validity rule (RFC 3550 A.2): datagram i -> its verdict, the first rule that fails
SX_HD int sx_rtcp_validate(const SxRtcpParseArgs& a, int i) {
    const SxRtpDgram d = a.dgrams[i];
    if (d.len < 4 || d.offset < 0 || (i64)d.offset + (i64)d.len > a.wire_bytes) return SX_RTCP_MALFORMED;
    const u8* lo = a.wire + d.offset;
    const u8* hi = lo + d.len;
    u32 h = sx_rtp_be32(lo, lo, hi);
    if ((h >> 30) != 2u) return SX_RTCP_VERSION;
    if (((h >> 29) & 1u) || (((h >> 16) & 255u) != 200u && ((h >> 16) & 255u) != 201u)) return SX_RTCP_FIRST_TYPE;
    i32 at = 0;
    while (at < d.len) {
        if (at + 4 > d.len) return SX_RTCP_LENGTH;
        h = sx_rtp_be32(lo + at, lo, hi);
        if ((h >> 30) != 2u) return SX_RTCP_VERSION;
        const i32 plen = 4 * (i32)((h & 0xFFFFu) + 1u);
        if ((i64)at + (i64)plen > (i64)d.len) return SX_RTCP_LENGTH;
        i32 body = plen - 4;
        if ((h >> 29) & 1u) {
            const i32 pad = (i32)hi[-1];
            if (at + plen != d.len || pad == 0 || (pad & 3) || pad > body) return SX_RTCP_LENGTH;
            body -= pad;
        }
        if (body < sx_rtcp_body_needed((h >> 16) & 255u, (h >> 24) & 31u)) return SX_RTCP_LENGTH;
        at += plen;
    }
    return SX_RTCP_ACCEPTED;
}
SX_HD i32 sx_rtcp_find(const u32* table, u32 ssrc, int n_streams) {
    const i32 s = sx_rtp_find_ssrc(table, ssrc);
    return s < n_streams ? s : -1;
}
// An ACCEPTED datagram, packet by packet.  vote: the atomics of the first pass and its counts (cnt [SX_RTCP_P_WORDS]); else the second
// pass, in which the winners write
SX_HD void sx_rtcp_process(const SxRtcpParseArgs& a, int i, bool vote, i32* cnt) {
    const SxRtpDgram d = a.dgrams[i];
    const u8* lo = a.wire + d.offset;
    const u8* hi = lo + d.len;
    const int n = a.n_streams;
    i32* sr_win = a.win; i32* fb_win = a.win + n; i32* fb_cnt = a.win + 2 * n; i32* bye = a.win + 3 * n;
    const u32 now_mid = sx_rtcp_mid32(sx_rtcp_now(a.d_now, a.now));
    i32 at = 0;
    while (at < d.len) {
        const u8* p = lo + at;
        const u32 h = sx_rtp_be32(p, lo, hi), pt = (h >> 16) & 255u, rc = (h >> 24) & 31u;
        if (pt == 200u || pt == 201u) {
            if (pt == 200u) {
                const i32 s = sx_rtcp_find(a.table_rx, sx_rtp_be32(p + 4, lo, hi), n);
                if (s < 0) {
                    if (vote) sx_rtcp_add(&cnt[SX_RTCP_P_UNKNOWN], 1);
                } else if (vote) {
                    sx_rtcp_max(&sr_win[s], i);
                    sx_rtcp_add(&cnt[SX_RTCP_P_SR], 1);
                } else if (sr_win[s] == i) {
                    SxRtcpRow& r = a.state[s];
                    r.lsr = (sx_rtp_be32(p + 8, lo, hi) << 16) | (sx_rtp_be32(p + 12, lo, hi) >> 16);
                    r.lsr_arrival = now_mid;
                    r.seen |= SX_RTCP_HAS_SR;
                }
            }
            const u8* blk = p + (pt == 200u ? 28 : 8);
            for (u32 b = 0; a.table_tx && b < rc; b++, blk += 24) {
                const i32 s = sx_rtcp_find(a.table_tx, sx_rtp_be32(blk, lo, hi), n);
                if (s < 0) continue;
                if (vote) {
                    sx_rtcp_max(&fb_win[s], i);
                    sx_rtcp_add(&fb_cnt[s], 1);
                    sx_rtcp_add(&cnt[SX_RTCP_P_BLOCKS], 1);
                } else if (fb_win[s] == i) {
                    SxRtcpFeedback* f = &a.feedback[s];
                    const u32 w1 = sx_rtp_be32(blk + 4, lo, hi);
                    f->fraction_lost = (i32)(w1 >> 24);
                    f->cum_lost = ((i32)(w1 << 8)) >> 8;
                    f->ext_high_seq = sx_rtp_be32(blk + 8, lo, hi);
                    f->jitter = sx_rtp_be32(blk + 12, lo, hi);
                    f->lsr = sx_rtp_be32(blk + 16, lo, hi);
                    f->dlsr = sx_rtp_be32(blk + 20, lo, hi);
                    const i32 rtt = (i32)(now_mid - f->lsr - f->dlsr);
                    f->rtt = f->lsr == 0 ? -1 : (rtt < 0 ? 0 : rtt);
                }
            }
        } else if (pt == 203u) {
            for (u32 b = 0; vote && b < rc; b++) {
                const i32 s = sx_rtcp_find(a.table_rx, sx_rtp_be32(p + 4 + 4 * b, lo, hi), n);
                if (s < 0) continue;
                sx_rtcp_or(&bye[s], 1);
                sx_rtcp_add(&cnt[SX_RTCP_P_BYE], 1);
            }
        } else if (vote) {
            sx_rtcp_add(&cnt[SX_RTCP_P_SKIPPED], 1);
        }
        at += 4 * (i32)((h & 0xFFFFu) + 1u);
    }
}
SX_HD void sx_rtcp_win_clear(const SxRtcpParseArgs& a, int s) {
    const int n = a.n_streams;
    a.win[s] = -1; a.win[n + s] = -1; a.win[2 * n + s] = 0; a.win[3 * n + s] = 0;
}
// row s of the feedback behind the votes: seen, and everything else where the row has no block (its winner writes the rest otherwise)
SX_HD void sx_rtcp_feedback_row(const SxRtcpParseArgs& a, int s) {
    const int n = a.n_streams;
    const i32 blocks = a.win[2 * n + s];
    SxRtcpFeedback* f = &a.feedback[s];
    f->seen = blocks | (a.win[3 * n + s] ? SOLO_RTCP_BYE : 0);
    if (blocks == 0) { f->fraction_lost = 0; f->cum_lost = 0; f->ext_high_seq = 0; f->jitter = 0; f->lsr = 0; f->dlsr = 0; f->rtt = -1; }
}
#if defined(__HIPCC__)
__global__ void __launch_bounds__(SX_RTCP_TILE) solo_rtcp_parse_begin_kernel(const SxRtcpParseArgs a) {
    const int s = (int)blockIdx.x * SX_RTCP_TILE + (int)threadIdx.x;
    if (s < a.n_streams) sx_rtcp_win_clear(a, s);
    if (blockIdx.x == 0 && threadIdx.x < SX_RTCP_P_WORDS) a.count[threadIdx.x] = 0;
}
__global__ void __launch_bounds__(SX_RTCP_TILE) solo_rtcp_vote_kernel(const SxRtcpParseArgs a) {
    __shared__ i32 cnt[SX_RTCP_P_WORDS];
    const int tid = (int)threadIdx.x, i = (int)blockIdx.x * SX_RTCP_TILE + tid;
    if (tid < SX_RTCP_P_WORDS) cnt[tid] = 0;
    __syncthreads();
    if (i < a.n_dgrams) {
        const int v = sx_rtcp_validate(a, i);
        a.ok[i] = v;
        atomicAdd(&cnt[v], 1);
        if (v == SX_RTCP_ACCEPTED) sx_rtcp_process(a, i, true, cnt);
    }
    __syncthreads();
    if (tid < SX_RTCP_P_WORDS && cnt[tid]) atomicAdd(&a.count[tid], cnt[tid]);
}
__global__ void __launch_bounds__(SX_RTCP_TILE) solo_rtcp_finish_kernel(const SxRtcpParseArgs a) {
    const int i = (int)blockIdx.x * SX_RTCP_TILE + (int)threadIdx.x;
    if (i < a.n_streams) sx_rtcp_feedback_row(a, i);
    if (i < a.n_dgrams && a.ok[i] == SX_RTCP_ACCEPTED) sx_rtcp_process(a, i, false, NULL);
}
static inline hipError_t solo_rtcp_parse_launch(const SxRtcpParseArgs& a, hipStream_t s) {
    const int row_tiles = (a.n_streams + SX_RTCP_TILE - 1) / SX_RTCP_TILE, n_tiles = (a.n_dgrams + SX_RTCP_TILE - 1) / SX_RTCP_TILE;
    hipLaunchKernelGGL(solo_rtcp_parse_begin_kernel, dim3((unsigned)row_tiles), dim3(SX_RTCP_TILE), 0, s, a);
    if (n_tiles > 0) hipLaunchKernelGGL(solo_rtcp_vote_kernel, dim3((unsigned)n_tiles), dim3(SX_RTCP_TILE), 0, s, a);
    hipLaunchKernelGGL(solo_rtcp_finish_kernel, dim3((unsigned)sx_max(row_tiles, n_tiles)), dim3(SX_RTCP_TILE), 0, s, a);
    return hipGetLastError();
}
#else
static inline void sx_rtcp_parse_host(SxRtcpParseArgs a) {
    std::vector<i32> win(4 * (size_t)a.n_streams), ok((size_t)a.n_dgrams + 1);
    i32 cnt[SX_RTCP_P_WORDS];
    for (int w = 0; w < SX_RTCP_P_WORDS; w++) cnt[w] = 0;
    a.win = win.data(); a.ok = ok.data();
    for (int s = 0; s < a.n_streams; s++) sx_rtcp_win_clear(a, s);
    for (int i = 0; i < a.n_dgrams; i++) {
        ok[i] = sx_rtcp_validate(a, i);
        cnt[ok[i]]++;
        if (ok[i] == SX_RTCP_ACCEPTED) sx_rtcp_process(a, i, true, cnt);
    }
    for (int s = 0; s < a.n_streams; s++) sx_rtcp_feedback_row(a, s);
    for (int i = a.n_dgrams - 1; i >= 0; i--)               // (any order will do: the votes are in)
        if (ok[i] == SX_RTCP_ACCEPTED) sx_rtcp_process(a, i, false, NULL);
    memcpy(a.count, cnt, sizeof(cnt));
}
#endif

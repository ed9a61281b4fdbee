// solo_api.hip -- the C ABI of libsolo_mi355x.so (include/solo_mi355x.h), the host-side pipelines behind it, and the decoder kernels of
// the 16 kHz API rate (solo_dec_kernels.h).  The encoder kernels and the 32 kHz decoder are reached through one launch table per build
// (solo_enc_ops.h, solo_dec_ops.h).
//
// Execution model: one 64-lane wavefront (= one workgroup) owns one stream and walks its packets in
// order; thousands of streams run concurrently.  Persistent codec state is an array of per-stream
// structs in HBM; the per-packet working set lives in LDS.  No host-side codec arithmetic exists in
// this library: without a usable HIP device every entry point fails.
#include <hip/hip_runtime.h>
#include <vector>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <new>

#include "../../include/solo_mi355x.h"
#include "solo_dec.h"

#define SOLO_CHECK(expr)                                        \
    do {                                                        \
        hipError_t e_ = (expr);                                 \
        if (e_ != hipSuccess) return -(int32_t)e_;              \
    } while (0)

// ---------------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------------
#include "solo_dec_kernels.h"
#include "solo_l0_probe.h"
#include "solo_send.h"          // the sender back end (solo_send_pack): rate-independent, compiled once, not a member of the launch tables
#include "solo_mix.h"           // the mixing bridge (solo_mix): likewise
#include "solo_mix_shared.h"    // ... with shared listener mixes (solo_mix_shared)
#include "solo_mix_selected.h"  // ... from a selection the caller brings (solo_mix_selected)
#include "solo_fanout.h"        // one source table, many destinations (solo_send_fanout)
#include "solo_recv_report.h"   // the read side of the receiver ring (solo_recv_report, solo_recv_track): likewise
#include "solo_migrate.h"       // stream states out of a handle and into another (solo_batch_export_streams / _import_streams): likewise
#include "solo_resample.h"      // PCM rate conversion between handles and towards 8 / 48 kHz endpoints (solo_resample): likewise
#include "solo_timescale.h"     // play-out time scaling by whole packets (solo_timescale): likewise
#include "solo_vad.h"           // voice activity, audio level and speaker selection of decoded rows (solo_vad, solo_vad_select): likewise
#include "solo_playout.h"       // adaptive play-out delay control (solo_playout_plan / _render / _tick): likewise
#include "solo_agc.h"           // level control and peak limiter of decoded rows (solo_agc): likewise
#include "solo_rows.h"          // the record kernels of those four objects (reset, listed reset, state copy): likewise
#include "solo_srtp.h"          // SRTP protection of the datagrams of solo_rtp.h (solo_srtp_protect / _unprotect): likewise
#include "solo_rtp.h"           // RTP framing of the sender's records and parsing of received datagrams (solo_rtp_pack / _parse): likewise
#include "solo_forward.h"       // forwarding without transcoding: levels per row from arrivals, routing under per-room slots (solo_forward_*): likewise
#include "solo_srtp_gcm.h"      // AEAD_AES_128_GCM for both (RFC 7714): the kernels behind theirs, the two key calls
#include "solo_srtcp.h"         // SRTCP protection of the compound packets of solo_rtcp.h (solo_srtcp_protect / _unprotect): likewise
#include "solo_rtcp.h"          // RTCP beside the RTP sessions: reception statistics, sender counts, compound packets out and in (solo_rtcp_*): likewise
#include "solo_rate.h"          // the sender's feedback loop: rate controller per row, its mode as a send mask (solo_rate_*): likewise

// conformance probe of the L0 fixed-point vocabulary as compiled for gfx950 (solo_debug_l0 below): out[i] = op(a[i], b[i], c[i])
__global__ void __launch_bounds__(64) solo_l0_probe_kernel(int op, int n, const i32* a, const i32* b, const i32* c, i32* out) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i < n) out[i] = sx_l0_probe(op, a[i], b[i], c[i]);
}
// SKP_Silk_sum_sqr_shift in its wave-cooperative form (solo_common.h): one wavefront per row of `len` samples
__global__ void __launch_bounds__(64) solo_sum_sqr_probe_kernel(const i16* x, int len, int stride, int odd_start, i32* energy, i32* shift) {
    __shared__ i16 buf[1024];
    const i16* row = x + (size_t)blockIdx.x * stride;
    SX_PAR(i, len) buf[i] = row[i];
    wv_sync();
    i32 e, s;
    sx_sum_sqr_shift_wv(&e, &s, buf, len, odd_start);
    if (SX_LANE == 0) { energy[blockIdx.x] = e; shift[blockIdx.x] = s; }
}

// conformance probe of the lane-crossing vocabulary of solo_wave.h in its 64-lane form, as this translation unit's kernels get it
// (solo_debug_waveops below): ONE wavefront per input vector of 64 words (v) and 64 second words (aux); a workgroup holds `wpb`
// wavefronts (1, or 4: the geometry of the front kernel), each with a vector of its own.  One output row of 64 words per result,
// EVERY lane stores its own copy: out[vector][row][lane].  No input reaches an address except the source lanes of wv_bcast and of
// the lane-register round trip, masked to 0 .. 63 (0 .. 127 samples) here.  The row numbers are restated by tests/wave_model.py.
// Mode 2 is the workgroup vocabulary (wg_sum, wg_scan_incl, wg_total), for wpb = 4 only: the four vectors of a workgroup are its 256
// lanes.  A wavefront whose vector lies beyond n_vec contributes zeros, stays for the barriers and stores nothing.
#define SOLO_WAVEOPS_ROWS0 27
#define SOLO_WAVEOPS_ROWS1 18
#define SOLO_WAVEOPS_ROWS2 3
// the chain of mode 1: every primitive consumes the result of the one before it, nothing else in between
#define SOLO_WAVEOPS_CHAIN(v)                                                                     \
    a = wv_sum(v);                                                                                \
    b = wv_max(sx_add(v, a));                                                                     \
    c = wv_min(v ^ b);                                                                            \
    d = wv_sum(sx_add(c, v));                                                                     \
    e = wv_scan_incl(sx_add(v, d));                                                               \
    f = e ^ v; g = lane; wv_argmin(&f, &g);                                                       \
    h = wv_sum64((i64)sx_mul(v, g));
__global__ void __launch_bounds__(256) solo_waveops_probe_kernel(int mode, int n_vec, int wpb, const i32* vin, const i32* auxin, i32* out) {
#if defined(__HIP_DEVICE_COMPILE__)                         // (the host pass has the 1-lane vocabulary: no lane registers, no column sum)
    const int vec = (int)blockIdx.x * wpb + (int)(threadIdx.x >> 6);
    if (mode == 2) {                                        // (mode is the launch's: every wavefront of the workgroup comes here)
        __shared__ i32 red[4], part[1][4];
        const bool live = vec < n_vec;
        const i32 x = live ? vin[(size_t)vec * 64 + SX_LANE] : 0;
        const i32 sum = wg_sum(x, red), incl = wg_scan_incl(x, part), total = wg_total(part[0]);
        if (live) {
            i32* o2 = out + (size_t)vec * SOLO_WAVEOPS_ROWS2 * 64 + SX_LANE;
            o2[0] = sum; o2[64] = incl; o2[128] = total;
        }
        return;
    }
    if (vec >= n_vec) return;                               // (whole wavefronts leave: every lane of a working wave stays active)
    const int lane = SX_LANE;
    const i32 v = vin[(size_t)vec * 64 + lane], aux = auxin[(size_t)vec * 64 + lane];
    const i32 aux0 = auxin[(size_t)vec * 64];               // lane 0's second word: source lane, rotation, seed, trip count
    i32* o = out + (size_t)vec * (mode == 0 ? SOLO_WAVEOPS_ROWS0 : SOLO_WAVEOPS_ROWS1) * 64 + lane;
#define ROW(r, x) o[(r) * 64] = (i32)(x)
    if (mode == 0) {
        ROW(0, wv_sum(v));
        ROW(1, wv_max(v));
        ROW(2, wv_min(v));
        ROW(3, wv_row_sum(v));
        ROW(4, wv_col_sum(v));
        const i64 s64 = wv_sum64((i64)(((u64)(u32)aux << 32) | (u32)v));
        ROW(5, (u32)s64);
        ROW(6, (u32)((u64)s64 >> 32));
        ROW(7, wv_scan_incl(v));
        i32 bv, bi;
        bv = v; bi = lane; wv_argmin(&bv, &bi); ROW(8, bv); ROW(9, bi);
        bv = v; bi = aux; wv_argmin(&bv, &bi); ROW(10, bv); ROW(11, bi);
        bv = v; bi = lane; wv_argmax(&bv, &bi); ROW(12, bv); ROW(13, bi);
        bv = v; bi = aux; wv_argmax(&bv, &bi); ROW(14, bv); ROW(15, bi);
        ROW(16, wv_bcast(v, aux0 & 63));
        ROW(17, wv_bcast(v, aux & 63));
        ROW(18, SX_UNI(wv_max(v)));
        {   // 128 samples in two lane registers (sample i: lane i & 63 of register i >> 6), deposited one by one, then fetched one by
            // one rotated by aux0 & 63 samples and deposited again
            const i32 rot = SX_UNI(aux0 & 63), key = SX_UNI(aux0);
            i32 w0 = 0, w1 = 0, r0 = 0, r1 = 0;
            for (int i = 0; i < 64; i++) {
                SX_WRLANE(w0, i, sx_mul(i + 1, (i32)0x9E3779B1u) ^ key);
                SX_WRLANE(w1, i, sx_mul(i + 65, (i32)0x9E3779B1u) ^ key);
            }
            for (int i = 0; i < 64; i++) {
                const int j0 = (i + rot) & 127, j1 = (i + 64 + rot) & 127;
                const i32 s0 = j0 < 64 ? SX_RDLANE(w0, j0 & 63) : SX_RDLANE(w1, j0 & 63);
                const i32 s1 = j1 < 64 ? SX_RDLANE(w0, j1 & 63) : SX_RDLANE(w1, j1 & 63);
                SX_WRLANE(r0, i, s0);
                SX_WRLANE(r1, i, s1);
            }
            ROW(19, r0);
            ROW(20, r1);
        }
        i32 z = sx_lcg_first(aux0);
        ROW(21, z);
        z = sx_lcg_next(z); ROW(22, z);
        z = sx_lcg_next(z); ROW(23, z);
        z = sx_lcg_next(z); ROW(24, z);
        // value, then index among the lanes that hold it (the selection rounds of solo_enc_analysis.h)
        const i32 vmin = wv_min(v);
        ROW(25, vmin);
        ROW(26, wv_min(v == vmin ? lane : SX_I32_MAX));
    } else {
        i32 a, b, c, d, e, f, g;
        i64 h;
        SOLO_WAVEOPS_CHAIN(v)
        ROW(0, a); ROW(1, b); ROW(2, c); ROW(3, d); ROW(4, e); ROW(5, f); ROW(6, g); ROW(7, (u32)h); ROW(8, (u32)((u64)h >> 32));
        // the same in a loop whose trip count only the input knows, every result fed back into the next round's vector
        const int trips = (aux0 & 7) + 1;
        i32 x = v;
        for (int t = 0; t < trips; t++) {
            if (t) x = sx_add(sx_add(x, a), sx_add(f, sx_add(g, (i32)(u32)h)));
            SOLO_WAVEOPS_CHAIN(x)
        }
        ROW(9, a); ROW(10, b); ROW(11, c); ROW(12, d); ROW(13, e); ROW(14, f); ROW(15, g); ROW(16, (u32)h); ROW(17, (u32)((u64)h >> 32));
    }
#undef ROW
#endif
}

// Subset calls: is the caller's device list strictly increasing inside [0, n_streams)?  One workgroup; the verdict word (0 = accepted)
// is the handle's (solo_batch::d_verdict), every kernel of the call reads it before it does anything (solo_stream_ctl.h).  A refused
// list also writes -1 to every status word of the call.
__global__ void __launch_bounds__(256) solo_stream_list_check_kernel(const i32* map, int n, int n_streams, u32* verdict, i32* status) {
    __shared__ int bad;
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    int mine = 0;
    for (int i = threadIdx.x; i < n; i += 256) {
        const i32 v = map[i];
        if (v < 0 || v >= n_streams || (i > 0 && map[i - 1] >= v)) mine = 1;
    }
    if (mine) atomicOr(&bad, 1);
    __syncthreads();
    const int verdict_bad = bad;
    if (threadIdx.x == 0) *verdict = (u32)verdict_bad;
    if (verdict_bad && status)
        for (int i = threadIdx.x; i < n; i += 256) status[i] = -1;
}

extern "C" const solo_dec_ops* solo_nb_dec_ops() { return &solo_dec_ops_table; }
extern "C" const solo_dec_ops* solo_wb_dec_ops();          // the same decoder compiled for the 32 kHz API rate (SILK wide band, 16 kHz bands): solo_api_wb.hip


// ---------------------------------------------------------------------------------------------------
// host side: handle + C ABI
// ---------------------------------------------------------------------------------------------------
// verdict words of subset calls (solo_stream_list_check_kernel), one per kind of call so that calls of different kinds in flight on
// different streams do not share one
enum {
    SOLO_VERDICT_ENC = 0,            // [0, 1] encode calls (by enc_seq: two can be in flight with asynchronous joins)
    SOLO_VERDICT_DEC = 2,            // decode
    SOLO_VERDICT_RING,               // receiver play-out
    SOLO_VERDICT_SEND,               // solo_send_pack_streams, solo_send_fanout (its source rows)
    SOLO_VERDICT_MIX,                // solo_mix, solo_mix_shared, solo_mix_selected (their room ids, slots, picks per room and packet)
    SOLO_VERDICT_REPORT,             // solo_recv_report
    SOLO_VERDICT_EXPORT,             // solo_batch_export_streams
    SOLO_VERDICT_RATES,              // solo_batch_update_rates
    SOLO_VERDICT_IMPORT,             // [9, 10] solo_batch_import_streams (its list, its records)
    SOLO_N_VERDICTS = SOLO_VERDICT_IMPORT + 2
};
// an environment knob that is a number
static int env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}
template <typename T>
static void dev_free(T*& p) {
    if (p) (void)hipFree(p);
    p = NULL;
}
// Grows a device scratch of the handle to `need` bytes (it never shrinks).  `s` is the stream whose kernels may still use the old
// buffer: growing synchronises it, steady-state calls do not.
static hipError_t grow_scratch(void*& p, size_t& bytes, size_t need, hipStream_t s) {
    if (need <= bytes) return hipSuccess;
    if (p) {
        const hipError_t e = hipStreamSynchronize(s);
        if (e != hipSuccess) return e;
        dev_free(p);
        bytes = 0;
    }
    const hipError_t e = hipMalloc(&p, need);
    if (e == hipSuccess) bytes = need;
    return e;
}
#ifdef SOLO_WITH_ENCODER
#include "solo_enc_ops.h"
extern "C" int solo_launch_gate(const unsigned int* flag, unsigned int target, void* hip_stream);      // solo_nsq_row.hip
extern "C" int solo_launch_gate_for(const unsigned int* flag, unsigned int target, int max_iters, void* hip_stream);
extern "C" const solo_enc_ops* solo_nb_enc_ops();                                                      // solo_enc_k.hip
extern "C" const solo_enc_ops* solo_wb_enc_ops();                                                      // solo_enc_k_wb.hip
#include "solo_enc_pipe.h"                                                                            // the encoder's launch schedule and what a handle owns for it
#endif

struct solo_batch {
    int32_t n_streams;
    int32_t slot;
    int have_enc, have_dec;
    USER_Ctrl_enc enc_ctrl;
    USER_Ctrl_dec dec_ctrl;
    void* d_enc_state;
#ifdef SOLO_WITH_ENCODER
    const solo_enc_ops* eops;        // launch table of the build that matches the encoder's rate (solo_enc_kernels.h)
    solo_enc_pipe enc;               // the encoder's streams, events, knobs, scratch and schedule state (solo_enc_pipe.h)
#endif
    // decoder: every kernel of a decode call runs on the caller's stream; two-kernel path: per chunk of packets the symbol extraction,
    // then the decoder proper
    hipEvent_t evDecDone;            // end of the most recent decode call, on whichever stream it was issued
    int dec_done_recorded;           // (a decode call has happened: evDecDone can be waited for)
    void* d_parsed;                  // extraction records of one chunk, grown on demand
    size_t parsed_bytes;
    int dec_pipe_ready, dec_split, dec_chunk, dec_first;
    size_t dec_scratch_cap;          // env SOLO_DEC_SCRATCH_CAP, read when the handle's decode pipeline is set up
    int timing;                      // solo_batch_set_timing: bracket every kernel with HIP events on its launch stream
    hipEvent_t evDec[2];             // brackets of a decode call on the caller's stream (the encoder's: solo_enc_pipe::tev)
    int ev_ready, ev_dec;
    const solo_dec_ops* dops;        // launch table of the build that matches the decoder's rate (solo_dec_kernels.h)
    void* d_dec_state;               // SxDecStream[n_streams] of that build
    // receiver staging ring (solo_recv.h): payload [N][D][2][slot] | length words [N][D] | play-out positions [N] | statistics
    uint8_t* d_recv_ring;
    uint32_t* d_recv_lens;
    int32_t* d_recv_play;
    uint32_t* d_recv_stats;
    int32_t recv_depth, recv_slot;
    // read side of the ring (solo_recv_report.h): per-stream counters [N][SX_RECV_TRK_WORDS] (allocated by the first solo_recv_track(1),
    // kept until the handle goes), the switch (counting happens only while it is on), and the selection flags [N] of a report call
    uint32_t* d_recv_trk;
    int recv_track;
    int32_t* d_recv_sel;
    uint32_t* d_verdict;             // [SOLO_N_VERDICTS], indexed by SOLO_VERDICT_*
    void* d_send_scratch;            // tile totals and tile bases of a solo_send_pack / solo_send_fanout call (solo_send.h, solo_fanout.h), grown on demand
    size_t send_scratch_bytes;
    void* d_mix_scratch;             // room plan, energies and flags of a solo_mix / solo_mix_shared call (solo_mix.h, solo_mix_shared.h), grown on demand
    size_t mix_scratch_bytes;
};

static int ctrl_hb_joint(int joint_enable, int joint_mode) { return joint_enable != 0 && joint_mode == 1; }
// AGR_BWE_SDK_API.c:119: the SILK core gets the target rate minus the high-band share, 1600 * 20 / bwe_framesize_ms
static int ctrl_silk_rate(const USER_Ctrl_enc* c) { return c->targetRate_bps - (ctrl_hb_joint(c->joint_enable, c->joint_mode) ? 800 : 1600); }
// joint_enable = 0, or joint_mode 1 (one 40 ms high-band frame per packet, AGR_BWE_SDK_API.c:64-67); the other joint modes are
// "reserved" in the reference as well
static bool ctrl_enc_supported(const USER_Ctrl_enc* c) {
    // framesize_ms 40 (two SILK frames per packet) or 20 (one: AGR_BWE_SDK_API.c:100-115, test/enc_main.c:129); the 40 ms high-band frame of
    // joint_mode 1 needs the 40 ms packet
    if (!(c->framesize_ms == 40 || (c->framesize_ms == 20 && c->joint_enable == 0)) || !(c->joint_enable == 0 || c->joint_mode == 1)) return false;
    if (c->samplerate == 16000) return true;
    // 32 kHz input: SILK runs wide band.  Below WB2MB_BITRATE_BPS (14 kbps for SILK = 15.6 kbps total, 14.8 kbps with the 40 ms
    // high-band frame) the reference starts at, or switches down to, 12 / 8 kHz internally (SKP_Silk_control_audio_bandwidth.c:44-76):
    // those rates and the switching are not built, so such a configuration is refused instead of coded differently
    USER_Ctrl_enc d = *c;
    if (d.targetRate_bps <= 0) d.targetRate_bps = 15600;
    return c->samplerate == 32000 && ctrl_silk_rate(&d) >= 14000;
}
static bool ctrl_dec_supported(const USER_Ctrl_dec* c) {
    // 32000: the wide-band decoder (solo_api_wb.hip); a stream whose internal rate is not 16 kHz is rejected packet by packet
    return (c->samplerate == 16000 || c->samplerate == 32000) && (c->framesize_ms == 40 || (c->framesize_ms == 20 && c->joint_enable == 0)) &&
           (c->joint_enable == 0 || c->joint_mode == 1);
}
// bytes of high band per packet: (QMF_HB_FrameSize / BWE_FrameSize) * HB_BYTE
static int ctrl_hb_bytes(int joint_enable, int joint_mode, int framesize_ms) { return (ctrl_hb_joint(joint_enable, joint_mode) || framesize_ms == 20) ? SX_HB_BYTES / 2 : SX_HB_BYTES; }
// SILK frames per packet, and the samples of a packet (JC1_FrameSize) given those of a 40 ms packet at the build's rate
static int ctrl_frames_per_packet(int framesize_ms) { return framesize_ms == 20 ? 1 : 2; }
static int ctrl_packet_samples(int samples_40ms, int framesize_ms) { return framesize_ms == 20 ? samples_40ms / 2 : samples_40ms; }
static int dec_packet_samples(const solo_batch* b) { return ctrl_packet_samples(b->dops->packet_samples, b->dec_ctrl.framesize_ms); }
// the decoder's hb_mode argument of sx_dec_state_init: bit 0 = joint_mode 1, bit 1 = one frame per packet
static int dec_hb_mode(const solo_batch* b) { return ctrl_hb_joint(b->dec_ctrl.joint_enable, b->dec_ctrl.joint_mode) | (ctrl_frames_per_packet(b->dec_ctrl.framesize_ms) == 1 ? 2 : 0); }

#ifdef SOLO_WITH_ENCODER
static int enc_hb_joint(const solo_batch* b) { return ctrl_hb_joint(b->enc_ctrl.joint_enable, b->enc_ctrl.joint_mode); }
static int enc_frames_per_packet(const solo_batch* b) { return ctrl_frames_per_packet(b->enc_ctrl.framesize_ms); }
static int enc_packet_samples(const solo_batch* b) { return ctrl_packet_samples(b->eops->packet_samples, b->enc_ctrl.framesize_ms); }
static int32_t solo_enc_reset(solo_batch* b, hipStream_t s) {
    SOLO_CHECK(b->eops->init(b->d_enc_state, b->n_streams, ctrl_silk_rate(&b->enc_ctrl), b->enc_ctrl.useMDIndex, enc_hb_joint(b),
                             b->enc_ctrl.dtx_enable ? 1 : 0, enc_frames_per_packet(b), s));
    return 0;
}
#endif

extern "C" {

const char* solo_version(void) { return "solo_mi355x 0.1 (gfx950)"; }

const char* solo_kernel_name(int32_t which) { return which == 0 ? "solo_nsq_kernel" : (which == 1 ? "solo_dec_synth_kernel" : (which == 2 ? "solo_enc_analysis_kernel" : "solo_enc_coding_kernel")); }

int32_t solo_batch_n_streams(const solo_batch_t* b) { return b ? b->n_streams : 0; }

// Kernel timing for benchmarks: when enabled every kernel launch of this handle is bracketed by HIP events on the launch
// stream; solo_batch_last_kernel_ms() synchronises on them and returns the durations of the most recent encode / decode call:
// ms[0] analysis, ms[1] quantiser, ms[2] coding, ms[3] decode (a field is -1 if that call has not happened yet).
int32_t solo_batch_set_timing(solo_batch_t* b, int32_t on) {
    if (!b) return -1;
    if (on && !b->ev_ready) {
        for (int i = 0; i < 2; i++) SOLO_CHECK(hipEventCreate(&b->evDec[i]));
        b->ev_ready = 1;
    }
#ifdef SOLO_WITH_ENCODER
    if (on) { SOLO_CHECK(enc_events_create(&b->enc.tev[0][0][0], 3 * SOLO_MAX_CHUNKS * 2, hipEventDefault)); b->enc.tev_ready = 1; }      // (those that are missing)
#endif
    b->timing = on ? 1 : 0;
    return 0;
}
int32_t solo_batch_last_kernel_ms(solo_batch_t* b, float* ms4) {
    if (!b || !ms4 || !b->ev_ready) return -1;
    for (int i = 0; i < 4; i++) ms4[i] = -1.0f;
#ifdef SOLO_WITH_ENCODER
    const solo_enc_pipe* p = &b->enc;
    if (p->ev_enc && p->tev_ready) {               // sum over the chunks (the three kernel types overlap in time)
        for (int k = 0; k < 3; k++) {
            float tot = 0.0f;
            for (int c = 0; c < p->last_chunks; c++) {
                float t = 0.0f;
                SOLO_CHECK(hipEventSynchronize(p->tev[k][c][1]));
                SOLO_CHECK(hipEventElapsedTime(&t, p->tev[k][c][0], p->tev[k][c][1]));
                tot += t;
            }
            ms4[k] = tot;
        }
    }
#endif
    if (b->ev_dec) {
        SOLO_CHECK(hipEventSynchronize(b->evDec[1]));
        SOLO_CHECK(hipEventElapsedTime(&ms4[3], b->evDec[0], b->evDec[1]));
    }
    return 0;
}
int32_t solo_batch_slot_bytes(const solo_batch_t* b) { return b ? b->slot : 0; }
// Makes `s` wait for the handle's encode work still in flight on its internal streams and for its most recent decode call (before
// init kernels overwrite states).
static int32_t solo_wait_in_flight(solo_batch_t* b, hipStream_t s) {
#ifdef SOLO_WITH_ENCODER
    // kernels of the most recent encode calls may still run on the internal streams (always so with async joins, and when
    // reset is issued on another stream than the encode was): the init kernels must not overtake them
    for (int which = 0; which < 2; which++) SOLO_CHECK(enc_pipe_wait(&b->enc, s, stream_capture(s), which, ENC_END));
#endif
    // (the most recent decode call may have been issued on another stream than `s`)
    if (b->dec_done_recorded) SOLO_CHECK(hipStreamWaitEvent(s, b->evDecDone, 0));
    return 0;
}

int32_t solo_batch_reset(solo_batch_t* b, void* hip_stream) {
    if (!b) return -1;
    hipStream_t s = (hipStream_t)hip_stream;
    {
        const int32_t r = solo_wait_in_flight(b, s);
        if (r) return r;
    }
    if (b->have_dec) SOLO_CHECK(b->dops->init(b->d_dec_state, b->n_streams, dec_hb_mode(b), b->dec_ctrl.useMDIndex, s));
#ifdef SOLO_WITH_ENCODER
    if (b->have_enc) {
        int32_t r = solo_enc_reset(b, s);
        if (r) return r;
    }
#endif
    return 0;
}

// Subset calls, of a handle (n_rows = its streams) or of a row-state object: the host checks only the count and the pointers (the list
// itself lives on the device: it is checked there, on the caller's stream, by solo_stream_list_check_kernel, whose verdict the call's
// kernels read).  No list (NULL = the identity): nothing to check, the call's kernels do not read the verdict
static hipError_t launch_list_check(const int32_t* d_list, int32_t n, int32_t n_rows, uint32_t* verdict, int32_t* d_status, hipStream_t s) {
    if (!d_list) return hipSuccess;
    hipLaunchKernelGGL(solo_stream_list_check_kernel, dim3(1), dim3(256), 0, s, d_list, n, n_rows, verdict, d_status);
    return hipGetLastError();
}
// every create call: this library has no CPU path
static bool have_device() {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0) return true;
    fprintf(stderr, "solo_mi355x: no HIP device available -- this library has no CPU path\n");
    return false;
}

// Per-stream controls of solo_batch_reset_streams and solo_batch_update_streams: everything is validated and turned into records
// (solo_stream_ctl.h) before anything is enqueued, so a refused call changes nothing.  Per stream: the encoder's rate, DTX and
// useMDIndex, the decoder's useMDIndex; samplerate, framesize_ms and the joint mode select the kernel build and the packet geometry
// and must be the handle's.  false: the call is refused.
static bool stream_ctl_records(const solo_batch* b, const int32_t* h_streams, int32_t n, int32_t which, const USER_Ctrl_enc* h_enc,
                               const USER_Ctrl_dec* h_dec, std::vector<SxStreamCtl>& er, std::vector<SxStreamCtl>& dr) {
    if (!b || which < 1 || which > 3 || !sx_list_ok(h_streams, n, b->n_streams)) return false;
    const bool do_enc = (which & 1) != 0, do_dec = (which & 2) != 0;
    if ((do_enc && !b->have_enc) || (do_dec && !b->have_dec) || (h_enc && !do_enc) || (h_dec && !do_dec)) return false;
    if (do_enc) {
        const USER_Ctrl_enc& he = b->enc_ctrl;
        er.resize((size_t)n);
        for (int32_t i = 0; i < n; i++) {
            USER_Ctrl_enc c = h_enc ? h_enc[i] : he;
            if (c.targetRate_bps <= 0) c.targetRate_bps = 15600;                    // AGR_BWE_SDK_API.c:35 (on a copy: the caller's array stays)
            if (c.samplerate != he.samplerate || c.framesize_ms != he.framesize_ms || c.joint_enable != he.joint_enable || c.joint_mode != he.joint_mode ||
                !ctrl_enc_supported(&c))
                return false;
            er[(size_t)i] = SxStreamCtl{h_streams[i], ctrl_silk_rate(&c), c.useMDIndex, c.dtx_enable ? 1 : 0};      // (c's joint mode is the handle's)
        }
    }
    if (do_dec) {
        const USER_Ctrl_dec& hd = b->dec_ctrl;
        dr.resize((size_t)n);
        for (int32_t i = 0; i < n; i++) {
            const USER_Ctrl_dec& c = h_dec ? h_dec[i] : hd;
            if (c.samplerate != hd.samplerate || c.framesize_ms != hd.framesize_ms || c.joint_enable != hd.joint_enable || c.joint_mode != hd.joint_mode ||
                !ctrl_dec_supported(&c))
                return false;
            dr[(size_t)i] = SxStreamCtl{h_streams[i], c.useMDIndex, 0, 0};
        }
    }
    return true;
}

// solo_batch_reset_streams (reinit: the listed streams start afresh) and solo_batch_update_streams (a running stream's control: the
// encoder's rate (setup_rate: the two SNR targets), DTX and useMDIndex, the decoder's useMDIndex; every other word of the states, the
// receiver ring and the play-out positions stay).  Records: stream_ctl_records.  The wait matters even more for an update than for a
// reset: the analysis / front kernels write a stream's whole SxEncState back when they end (an update that overtook them would be
// undone), and the coder reads useDTX / useMDIndex of the packets it codes.
static int32_t stream_ctl_apply(solo_batch_t* b, bool reinit, const int32_t* h_streams, int32_t n, int32_t which, const USER_Ctrl_enc* h_enc,
                                const USER_Ctrl_dec* h_dec, hipStream_t s) {
    std::vector<SxStreamCtl> er, dr;
    if (!stream_ctl_records(b, h_streams, n, which, h_enc, h_dec, er, dr)) return -1;
    {
        const int32_t r = solo_wait_in_flight(b, s);
        if (r) return r;
    }
    if (!dr.empty()) SOLO_CHECK(reinit ? b->dops->init_list(b->d_dec_state, dr.data(), n, dec_hb_mode(b), s) : b->dops->ctl_list(b->d_dec_state, dr.data(), n, s));
#ifdef SOLO_WITH_ENCODER
    if (!er.empty())
        SOLO_CHECK(reinit ? b->eops->init_list(b->d_enc_state, er.data(), n, enc_hb_joint(b), enc_frames_per_packet(b), s)
                          : b->eops->ctl_list(b->d_enc_state, er.data(), n, s));
#endif
    return 0;
}
int32_t solo_batch_reset_streams(solo_batch_t* b, const int32_t* h_streams, int32_t n, int32_t which, const USER_Ctrl_enc* h_enc,
                                 const USER_Ctrl_dec* h_dec, void* hip_stream) {
    return stream_ctl_apply(b, true, h_streams, n, which, h_enc, h_dec, (hipStream_t)hip_stream);
}
int32_t solo_batch_update_streams(solo_batch_t* b, const int32_t* h_streams, int32_t n, int32_t which, const USER_Ctrl_enc* h_enc,
                                  const USER_Ctrl_dec* h_dec, void* hip_stream) {
    return stream_ctl_apply(b, false, h_streams, n, which, h_enc, h_dec, (hipStream_t)hip_stream);
}

// A running stream's rate from DEVICE memory (include/solo_mi355x.h; the kernel: solo_enc_rate_list_kernel of the handle's build).  The
// wait is that of solo_batch_update_streams, for its reason; the values are judged on the device (sx_enc_apply_target), the list by the
// list check kernel.
int32_t solo_batch_update_rates(solo_batch_t* b, const int32_t* d_streams, int32_t n, const int32_t* d_target_bps, solo_rate_apply_count_t* d_count,
                                void* hip_stream) {
    if (!b || !sx_rate_apply_call_ok(b->n_streams, b->have_enc != 0, d_streams, n, d_target_bps, d_count)) return -1;
#ifdef SOLO_WITH_ENCODER
    hipStream_t st = (hipStream_t)hip_stream;
    {
        const int32_t r = solo_wait_in_flight(b, st);
        if (r) return r;
    }
    uint32_t* verdict = b->d_verdict + SOLO_VERDICT_RATES;
    SOLO_CHECK(launch_list_check(d_streams, n, b->n_streams, verdict, NULL, st));
    SOLO_CHECK(b->eops->rate_list(b->d_enc_state, d_streams, d_target_bps, n, enc_hb_joint(b), d_count, verdict, st));
    return 0;
#else
    return -1;
#endif
}

solo_batch_t* solo_batch_create(int32_t n_streams, const USER_Ctrl_enc* enc, const USER_Ctrl_dec* dec, int32_t slot_bytes) {
    if (n_streams <= 0 || !have_device()) return NULL;
    if (enc && !ctrl_enc_supported(enc)) return NULL;
    if (dec && !ctrl_dec_supported(dec)) return NULL;
    solo_batch* b = new (std::nothrow) solo_batch();
    if (!b) return NULL;
    memset(b, 0, sizeof(*b));
    b->n_streams = n_streams;
    b->slot = slot_bytes > 0 ? slot_bytes : SOLO_DEFAULT_SLOT_BYTES;
    if (enc) {
#ifdef SOLO_WITH_ENCODER
        b->have_enc = 1;
        b->enc_ctrl = *enc;
        if (b->enc_ctrl.targetRate_bps <= 0) b->enc_ctrl.targetRate_bps = 15600;  // AGR_BWE_SDK_API.c:35
        b->eops = enc->samplerate == 32000 ? solo_wb_enc_ops() : solo_nb_enc_ops();
        if (hipMalloc(&b->d_enc_state, b->eops->state_bytes * (size_t)n_streams) != hipSuccess) { solo_batch_destroy(b); return NULL; }
#else
        delete b;
        return NULL;
#endif
    }
    if (dec) {
        b->have_dec = 1;
        b->dec_ctrl = *dec;
        b->dops = dec->samplerate == 32000 ? solo_wb_dec_ops() : solo_nb_dec_ops();
        if (enc && enc->samplerate != dec->samplerate) { solo_batch_destroy(b); return NULL; }     // a handle has one rate
        if (hipMalloc(&b->d_dec_state, b->dops->state_bytes * (size_t)n_streams) != hipSuccess) { solo_batch_destroy(b); return NULL; }
    }
    if (hipMalloc((void**)&b->d_verdict, SOLO_N_VERDICTS * sizeof(uint32_t)) != hipSuccess || hipMemset(b->d_verdict, 0, SOLO_N_VERDICTS * sizeof(uint32_t)) != hipSuccess) {
        solo_batch_destroy(b);
        return NULL;
    }
    if (solo_batch_reset(b, NULL) != 0 || hipDeviceSynchronize() != hipSuccess) { solo_batch_destroy(b); return NULL; }
    return b;
}

static void solo_recv_free(solo_batch_t* b);
void solo_batch_destroy(solo_batch_t* b) {
    if (!b) return;
    solo_recv_free(b);
    dev_free(b->d_recv_trk);
    if (b->dec_pipe_ready) (void)hipEventDestroy(b->evDecDone);
    dev_free(b->d_parsed);
    dev_free(b->d_dec_state);
    dev_free(b->d_verdict);
    dev_free(b->d_send_scratch);
    dev_free(b->d_mix_scratch);
    if (b->ev_ready) for (int i = 0; i < 2; i++) (void)hipEventDestroy(b->evDec[i]);
#ifdef SOLO_WITH_ENCODER
    enc_pipe_destroy(&b->enc);
    dev_free(b->d_enc_state);
#endif
    delete b;
}

// Chunks of the two-kernel decoder.  A call runs on the caller's stream, chunk after chunk: the extraction of a chunk's symbols, then
// the decoder proper over the same packets, both on ONE buffer of records.  Nothing overlaps, and nothing could: the two kernels never
// share a compute unit (the synthesis kernel's 16 workgroups take all of its LDS and registers), so an extraction running ahead on a
// stream of its own would hide nothing.  Every chunk boundary only costs: a synthesis launch reloads and stores 4096 stream states,
// and its last workgroups run in a thinly populated tail.  Measured (4096 streams x 50 packets): chunks of 24 packets after a first
// one of 4: 9.0 ms; 6 + 44: 7.7 ms; ONE chunk: 7.4 ms (8192 streams, 30 % description loss: 17.5 / 16.2 / 16.0 ms).  So a call is
// one chunk up to 64 packets (the extraction records of a chunk are 2216 B per packet: 581 MB for 4096 streams x 64 packets), longer
// calls are cut into chunks of 64; chunks exist to bound that buffer, not to gain time.
#define SOLO_DEC_FIRST_CHUNK 64
#define SOLO_DEC_CHUNK_DEFAULT 64
static_assert(2 * sizeof(SxExtracted) + 8 == 2216, "include/solo_mi355x.h documents 2216 bytes of extraction records (2 x 1104 B + two list entries) per packet (16 kHz API rate)");
// one-time set-up of a handle's decode pipeline: the knobs and the event that marks the end of a decode call
static int32_t solo_dec_pipe_setup(solo_batch* b) {
    b->dec_split = env_int("SOLO_DEC_SPLIT", 1);
    if (ctrl_frames_per_packet(b->dec_ctrl.framesize_ms) == 1) b->dec_split = 0;      // (the extraction records describe two-frame packets)
    b->dec_chunk = env_int("SOLO_DEC_CHUNK", SOLO_DEC_CHUNK_DEFAULT);
    if (b->dec_chunk <= 0) b->dec_chunk = 1 << 30;
    b->dec_first = env_int("SOLO_DEC_FIRST_CHUNK", SOLO_DEC_FIRST_CHUNK);
    if (b->dec_first <= 0) b->dec_first = SOLO_DEC_FIRST_CHUNK;
    // (read per handle like the other SOLO_DEC_* knobs; a value that does not parse to a positive number means the default)
    const char* e = getenv("SOLO_DEC_SCRATCH_CAP");
    b->dec_scratch_cap = e ? (size_t)strtoull(e, NULL, 10) : 0;
    if (b->dec_scratch_cap == 0) b->dec_scratch_cap = (size_t)1 << 30;
    SOLO_CHECK(hipEventCreateWithFlags(&b->evDecDone, hipEventDisableTiming));
    b->dec_pipe_ready = 1;
    return 0;
}
// Two kernels, chunk by chunk on `st`: the symbols of every description of a chunk of packets are read off the range coder at once, one
// lane each (X_c); the decoder proper, one wavefront per stream, packets in order, follows on the same record buffer (D_c).  Stream order
// is all the ordering there is: X_c after D_{c-1} (the buffer is free again), D_c after X_c.
static hipError_t solo_decode_chunks(solo_batch_t* b, const int32_t* map, int ns, const uint32_t* verdict, const uint8_t* d_bits, const int16_t* d_nbytes,
                                     const uint8_t* d_recv, int32_t n_packets, int16_t* d_pcm, int32_t* d_status, hipStream_t st) {
    // packets per chunk: the knob, capped so that the buffer of extraction records stays below SOLO_DEC_SCRATCH_CAP bytes (default 1 GiB;
    // the records are 2216 B per packet at the 16 kHz API rate: 4096 streams x 64 packets = 581 MB, 65536 streams -> 7 packets per chunk).
    // include/solo_mi355x.h states the footprint.
    const size_t rec_bytes = b->dops->extracted_bytes;
    int cp = n_packets < b->dec_chunk ? n_packets : b->dec_chunk;
    {   // (floor: one packet per chunk -- a handle with more than cap / 2216 streams holds n_streams x 2216 B, see the header)
        const size_t fit = b->dec_scratch_cap / ((size_t)ns * rec_bytes);
        if ((size_t)cp > fit) cp = fit < 1 ? 1 : (int)fit;
    }
    // (a first chunk of SOLO_DEC_FIRST_CHUNK packets where the call is longer than two of them; never larger than the buffer: c0 <= cp)
    const int c0 = (n_packets > 2 * b->dec_first && cp > b->dec_first) ? b->dec_first : cp;
    const int nchunks = 1 + (n_packets - c0 + cp - 1) / cp;
    const size_t need = (size_t)ns * (size_t)cp * rec_bytes + 256;      // (+ the count of the listed description slots)
    if (need > b->parsed_bytes && b->dec_done_recorded) {
        // (belt and braces: `st` already waits for the previous call, on whichever stream that was issued, and growing synchronises `st`)
        const hipError_t e = hipEventSynchronize(b->evDecDone);
        if (e != hipSuccess) return e;
    }
    hipError_t lerr = grow_scratch(b->d_parsed, b->parsed_bytes, need, st);
    for (int c = 0; c < nchunks && lerr == hipSuccess; c++) {
        const int p0 = c == 0 ? 0 : c0 + (c - 1) * cp, pc = c == 0 ? c0 : ((p0 + cp <= n_packets) ? cp : n_packets - p0);
        lerr = b->dops->extract(b->d_dec_state, d_bits, d_nbytes, d_recv, ns, n_packets, p0, pc, b->slot, b->d_parsed, map, verdict, st);
        if (lerr != hipSuccess) break;
        lerr = b->dops->synth(b->d_dec_state, d_bits, d_nbytes, d_recv, ns, n_packets, p0, pc, b->slot, b->d_parsed, d_pcm, d_status, map, verdict, st);
    }
    return lerr;
}
// map = NULL: every stream (solo_batch_decode); else the n listed streams of solo_batch_decode_streams, their records / PCM / status compact
static int32_t solo_decode_impl(solo_batch_t* b, const int32_t* map, int32_t n, const uint8_t* d_bits, const int16_t* d_nbytes, const uint8_t* d_recv,
                                int32_t n_packets, int16_t* d_pcm, int32_t* d_status, hipStream_t st) {
    const int ns = map ? n : b->n_streams;
    uint32_t* verdict = map ? b->d_verdict + SOLO_VERDICT_DEC : NULL;
    const bool tm = b->timing && b->ev_ready;
    if (!b->dec_pipe_ready) {
        const int32_t r = solo_dec_pipe_setup(b);
        if (r) return r;
    }
    // the previous decode call may have been issued on ANOTHER stream than this one: it used the same states, record buffer and verdict word
    if (b->dec_done_recorded) SOLO_CHECK(hipStreamWaitEvent(st, b->evDecDone, 0));
    if (tm) (void)hipEventRecord(b->evDec[0], st);
    hipError_t lerr = launch_list_check(map, n, b->n_streams, verdict, d_status, st);
    if (lerr == hipSuccess && b->dec_split)
        lerr = solo_decode_chunks(b, map, ns, verdict, d_bits, d_nbytes, d_recv, n_packets, d_pcm, d_status, st);
    else if (lerr == hipSuccess)         // single kernel: one wavefront per stream parses (two lanes) and synthesises
        lerr = b->dops->decode(b->d_dec_state, d_bits, d_nbytes, d_recv, ns, n_packets, b->slot, d_pcm, d_status, map, verdict, st);
    // (also after a refused launch: what was enqueued still runs)
    if (hipEventRecord(b->evDecDone, st) == hipSuccess) b->dec_done_recorded = 1;
    if (tm) { (void)hipEventRecord(b->evDec[1], st); b->ev_dec = 1; }
    SOLO_CHECK(lerr);
    return 0;
}
int32_t solo_batch_decode(solo_batch_t* b, const uint8_t* d_bits, const int16_t* d_nbytes, const uint8_t* d_recv,
                          int32_t n_packets, int16_t* d_pcm, int32_t* d_status, void* hip_stream) {
    if (!b || !b->have_dec || !d_bits || !d_nbytes || !d_pcm || n_packets <= 0) return -1;
    return solo_decode_impl(b, NULL, 0, d_bits, d_nbytes, d_recv, n_packets, d_pcm, d_status, (hipStream_t)hip_stream);
}
int32_t solo_batch_decode_streams(solo_batch_t* b, const int32_t* d_streams, int32_t n, const uint8_t* d_bits, const int16_t* d_nbytes,
                                  const uint8_t* d_recv, int32_t n_packets, int16_t* d_pcm, int32_t* d_status, void* hip_stream) {
    if (!b || !b->have_dec || !d_streams || n <= 0 || n > b->n_streams || !d_bits || !d_nbytes || !d_pcm || n_packets <= 0) return -1;
    return solo_decode_impl(b, d_streams, n, d_bits, d_nbytes, d_recv, n_packets, d_pcm, d_status, (hipStream_t)hip_stream);
}

int32_t solo_batch_decode_split(solo_batch_t* b, const uint8_t* d_descA, const int16_t* d_lenA, const uint8_t* d_descB,
                                const int16_t* d_lenB, int32_t slot_bytes, int32_t n_packets, int16_t* d_pcm, int32_t* d_status,
                                void* hip_stream) {
    if (!b || !b->have_dec || !d_descA || !d_lenA || !d_descB || !d_lenB || !d_pcm || n_packets <= 0 || slot_bytes <= 0) return -1;
    SOLO_CHECK(b->dops->split(b->d_dec_state, d_descA, d_lenA, d_descB, d_lenB, b->n_streams, n_packets, slot_bytes, d_pcm, d_status, (hipStream_t)hip_stream));
    return 0;
}

// ---- receiver staging ring (solo_recv.h) ---------------------------------------------------------------------------------------
static void solo_recv_free(solo_batch_t* b) {
    dev_free(b->d_recv_ring);
    dev_free(b->d_recv_lens);
    dev_free(b->d_recv_play);
    dev_free(b->d_recv_stats);
    dev_free(b->d_recv_sel);
    b->recv_depth = b->recv_slot = 0;
}
int32_t solo_recv_create(solo_batch_t* b, int32_t depth, int32_t slot_bytes, int32_t first_seq, void* hip_stream) {
    if (!b || !b->have_dec || depth <= 0 || depth > 4096 || slot_bytes <= 0 || slot_bytes > 0x7FFF || first_seq < 0) return -1;
    hipStream_t st = (hipStream_t)hip_stream;
    if (depth != b->recv_depth || slot_bytes != b->recv_slot) {
        SOLO_CHECK(hipStreamSynchronize(st));
        solo_recv_free(b);
        const size_t ne = (size_t)b->n_streams * (size_t)depth;
        hipError_t e = hipMalloc((void**)&b->d_recv_ring, ne * 2 * (size_t)slot_bytes);
        if (e == hipSuccess) e = hipMalloc((void**)&b->d_recv_lens, ne * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMalloc((void**)&b->d_recv_play, (size_t)b->n_streams * sizeof(int32_t));
        if (e == hipSuccess) e = hipMalloc((void**)&b->d_recv_stats, SX_RECV_NSTATS * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMalloc((void**)&b->d_recv_sel, (size_t)b->n_streams * sizeof(int32_t));      // (so that solo_recv_report allocates nothing)
        if (e != hipSuccess) { solo_recv_free(b); return -(int32_t)e; }
        b->recv_depth = depth; b->recv_slot = slot_bytes;
    }
    SOLO_CHECK(solo_recv_launch_reset(b->d_recv_lens, b->d_recv_play, b->d_recv_stats, b->n_streams, depth, first_seq, st));
    if (b->d_recv_trk) SOLO_CHECK(solo_recv_trk_reset_launch(b->d_recv_trk, b->n_streams, depth, st));
    return 0;
}
int32_t solo_recv_reset_streams(solo_batch_t* b, const int32_t* h_streams, int32_t n, const int32_t* h_first_seq, void* hip_stream) {
    if (!b || !b->d_recv_ring || !h_first_seq || !sx_list_ok(h_streams, n, b->n_streams)) return -1;
    std::vector<SxStreamCtl> rr((size_t)n);
    for (int32_t i = 0; i < n; i++) {
        if (h_first_seq[i] < 0) return -1;
        rr[(size_t)i] = SxStreamCtl{h_streams[i], h_first_seq[i], 0, 0};
    }
    SOLO_CHECK(solo_recv_launch_reset_list(b->d_recv_lens, b->d_recv_play, rr.data(), n, b->recv_depth, (hipStream_t)hip_stream));
    if (b->d_recv_trk) SOLO_CHECK(solo_recv_trk_reset_list_launch(b->d_recv_trk, rr.data(), n, b->recv_depth, (hipStream_t)hip_stream));   // (a new call joins the slot)
    return 0;
}
int32_t solo_recv_insert(solo_batch_t* b, const solo_arrival_t* d_arrivals, int32_t n_arrivals, const uint8_t* d_payload, int64_t payload_bytes,
                         void* hip_stream) {
    if (!b || !b->d_recv_ring || n_arrivals < 0 || (n_arrivals > 0 && (!d_arrivals || !d_payload)) || payload_bytes < 0) return -1;
    if (n_arrivals == 0) return 0;
    // (desc = -1 is accepted for the streams whose decoder runs with useMDIndex = 1: the kernel reads each stream's own flag)
    SOLO_CHECK(b->dops->recv_insert(d_arrivals, n_arrivals, d_payload, (long long)payload_bytes, b->n_streams, b->recv_depth, b->recv_slot, b->d_dec_state,
                                    b->d_recv_ring, b->d_recv_lens, b->d_recv_play, b->d_recv_stats, b->recv_track ? b->d_recv_trk : NULL,
                                    (hipStream_t)hip_stream));
    return 0;
}
int32_t solo_recv_decode(solo_batch_t* b, int32_t n_packets, int16_t* d_pcm, int32_t* d_status, void* hip_stream) {
    if (!b || !b->d_recv_ring || !d_pcm || n_packets <= 0 || n_packets > b->recv_depth) return -1;
    if (b->recv_track)            // what the packets about to be played are made of (solo_recv_report.h), ahead of the kernel that clears them
        SOLO_CHECK(solo_recv_account_launch(b->d_recv_lens, b->d_recv_play, b->d_recv_trk, b->n_streams, n_packets, b->recv_depth, NULL, NULL, (hipStream_t)hip_stream));
    SOLO_CHECK(b->dops->ring(b->d_dec_state, b->d_recv_ring, b->d_recv_lens, b->d_recv_play, b->n_streams, n_packets, b->recv_depth, b->recv_slot, d_pcm,
                             d_status, NULL, NULL, (hipStream_t)hip_stream));
    return 0;
}
int32_t solo_recv_decode_streams(solo_batch_t* b, const int32_t* d_streams, int32_t n, int32_t n_packets, int16_t* d_pcm, int32_t* d_status,
                                 void* hip_stream) {
    if (!b || !b->d_recv_ring || !d_streams || n <= 0 || n > b->n_streams || !d_pcm || n_packets <= 0 || n_packets > b->recv_depth) return -1;
    hipStream_t st = (hipStream_t)hip_stream;
    uint32_t* verdict = b->d_verdict + SOLO_VERDICT_RING;
    SOLO_CHECK(launch_list_check(d_streams, n, b->n_streams, verdict, d_status, st));
    if (b->recv_track) SOLO_CHECK(solo_recv_account_launch(b->d_recv_lens, b->d_recv_play, b->d_recv_trk, n, n_packets, b->recv_depth, d_streams, verdict, st));
    SOLO_CHECK(b->dops->ring(b->d_dec_state, b->d_recv_ring, b->d_recv_lens, b->d_recv_play, n, n_packets, b->recv_depth, b->recv_slot, d_pcm, d_status,
                             d_streams, verdict, st));
    return 0;
}
int32_t solo_recv_stats(solo_batch_t* b, uint32_t* out8, void* hip_stream) {
    if (!b || !b->d_recv_ring || !out8) return -1;
    SOLO_CHECK(hipMemcpyAsync(out8, b->d_recv_stats, SX_RECV_NSTATS * sizeof(uint32_t), hipMemcpyDeviceToHost, (hipStream_t)hip_stream));
    SOLO_CHECK(hipStreamSynchronize((hipStream_t)hip_stream));
    return 0;
}

// ---- read side of the ring (solo_recv_report.h): per-stream counters, queue report, play-out list ----------------------------------
int32_t solo_recv_track(solo_batch_t* b, int32_t on, void* hip_stream) {
    if (!b || !b->d_recv_ring) return -1;
    if (!on) { b->recv_track = 0; return 0; }               // (the values stay; solo_recv_report goes on showing them)
    if (!b->d_recv_trk) {
        const hipError_t e = hipMalloc((void**)&b->d_recv_trk, (size_t)b->n_streams * SX_RECV_TRK_WORDS * sizeof(uint32_t));
        if (e != hipSuccess) { b->d_recv_trk = NULL; return -(int32_t)e; }
    }
    SOLO_CHECK(solo_recv_trk_reset_launch(b->d_recv_trk, b->n_streams, b->recv_depth, (hipStream_t)hip_stream));
    b->recv_track = 1;
    return 0;
}
int32_t solo_recv_report(solo_batch_t* b, const int32_t* d_streams, int32_t n, const int32_t* d_min_ready, int32_t min_ready, int32_t max_span,
                         int32_t flags, solo_recv_report_t* d_reports, int32_t* d_play_list, int32_t* d_play_rows, solo_recv_report_count_t* d_count,
                         void* hip_stream) {
    if (!b || !b->d_recv_ring || n <= 0 || n > b->n_streams || (!d_streams && n != b->n_streams)) return -1;
    if ((!d_reports && !d_play_list && !d_play_rows) || ((d_play_list || d_play_rows) && !d_count) || (flags & ~SOLO_RECV_REPORT_CLEAR_MARGIN)) return -1;
    if ((uintptr_t)d_reports & 15) return -1;               // (the records are stored 16 bytes at a time)
    hipStream_t st = (hipStream_t)hip_stream;
    uint32_t* verdict = b->d_verdict + SOLO_VERDICT_REPORT;
    SOLO_CHECK(launch_list_check(d_streams, n, b->n_streams, verdict, NULL, st));
    SxRecvReportArgs a;
    a.lens = b->d_recv_lens; a.play = b->d_recv_play; a.trk = b->d_recv_trk; a.map = d_streams; a.min_ready_v = d_min_ready;
    a.reports = (uint32_t*)d_reports; a.sel = b->d_recv_sel;
    a.n = n; a.depth = b->recv_depth; a.min_ready = min_ready; a.max_span = max_span; a.clear_margin = (flags & SOLO_RECV_REPORT_CLEAR_MARGIN) != 0;
    SOLO_CHECK(solo_recv_report_launch(a, d_play_list, d_play_rows, d_count, verdict, st));
    return 0;
}

// ---- the handle's geometry, for the bridge stages below (they run no codec kernel: the handle lends them its geometry and its scratch) ----
// samples of a packet and, where asked for, the sample rate: the decoder's, or the encoder's when the handle has no decoder; 0 when it
// has neither
static int handle_packet_samples(const solo_batch* b, int* fs = NULL) {
    int L = 0, rate = 0;
    if (b->have_dec) { L = dec_packet_samples(b); rate = b->dec_ctrl.samplerate; }
#ifdef SOLO_WITH_ENCODER
    else if (b->have_enc) { L = enc_packet_samples(b); rate = b->enc_ctrl.samplerate; }
#endif
    if (fs) *fs = rate;
    return L;
}
// high-band bytes of a packet: the encoder's, or the decoder's when the handle has no encoder
static int handle_hb_bytes(const solo_batch* b) {
    return b->have_enc ? ctrl_hb_bytes(b->enc_ctrl.joint_enable, b->enc_ctrl.joint_mode, b->enc_ctrl.framesize_ms)
                       : ctrl_hb_bytes(b->dec_ctrl.joint_enable, b->dec_ctrl.joint_mode, b->dec_ctrl.framesize_ms);
}

// ---- sender back end (solo_send.h): slots + length records -> datagram records + a dense payload pool ----------------------------
// map = NULL: the rows are the handle's streams 0 .. n - 1; else row i is stream map[i] (checked on the device, ahead of the passes)
static int32_t solo_send_impl(solo_batch_t* b, const int32_t* map, int32_t n, const uint8_t* d_bits, const int16_t* d_nbytes, const uint8_t* d_send,
                              int32_t n_packets, const int32_t* d_seq_base, int32_t first_seq, solo_arrival_t* d_records, int32_t max_records,
                              uint8_t* d_payload, int64_t payload_capacity, solo_send_count_t* d_count, hipStream_t st) {
    if (!d_bits || !d_nbytes || !d_records || !d_payload || !d_count || n_packets <= 0 || max_records < 0 || payload_capacity < 0) return -1;
    if ((int64_t)n * (int64_t)n_packets * 2 >= ((int64_t)1 << 31)) return -1;
    SOLO_CHECK(grow_scratch(b->d_send_scratch, b->send_scratch_bytes, solo_send_scratch_bytes(n * n_packets), st));
    uint32_t* verdict = b->d_verdict + SOLO_VERDICT_SEND;
    SOLO_CHECK(launch_list_check(map, n, b->n_streams, verdict, NULL, st));
    SxSendArgs a;
    a.bits = d_bits; a.nbytes = d_nbytes; a.send = d_send; a.seq_base = d_seq_base; a.map = map;
    a.n = n; a.n_packets = n_packets; a.slot = b->slot; a.hbb = handle_hb_bytes(b); a.first_seq = first_seq;
    SOLO_CHECK(solo_send_launch(a, b->d_send_scratch, d_records, max_records, d_payload, (long long)payload_capacity, d_count, verdict, st));
    return 0;
}
int32_t solo_send_pack(solo_batch_t* b, const uint8_t* d_bits, const int16_t* d_nbytes, const uint8_t* d_send, int32_t n_packets,
                       const int32_t* d_seq_base, int32_t first_seq, solo_arrival_t* d_records, int32_t max_records, uint8_t* d_payload,
                       int64_t payload_capacity, solo_send_count_t* d_count, void* hip_stream) {
    if (!b) return -1;
    return solo_send_impl(b, NULL, b->n_streams, d_bits, d_nbytes, d_send, n_packets, d_seq_base, first_seq, d_records, max_records, d_payload,
                          payload_capacity, d_count, (hipStream_t)hip_stream);
}
int32_t solo_send_pack_streams(solo_batch_t* b, const int32_t* d_streams, int32_t n, const uint8_t* d_bits, const int16_t* d_nbytes,
                               const uint8_t* d_send, int32_t n_packets, const int32_t* d_seq_base, int32_t first_seq, solo_arrival_t* d_records,
                               int32_t max_records, uint8_t* d_payload, int64_t payload_capacity, solo_send_count_t* d_count, void* hip_stream) {
    if (!b || !d_streams || n <= 0 || n > b->n_streams) return -1;
    return solo_send_impl(b, d_streams, n, d_bits, d_nbytes, d_send, n_packets, d_seq_base, first_seq, d_records, max_records, d_payload,
                          payload_capacity, d_count, (hipStream_t)hip_stream);
}

// one source table, many destinations (solo_fanout.h); the handle lends its geometry and its scratch, as above
int32_t solo_send_fanout(solo_batch_t* b, const uint8_t* d_bits, const int16_t* d_nbytes, int32_t n_src, const int32_t* d_source, const int32_t* d_dst_stream,
                         int32_t n_dst, const uint8_t* d_send, int32_t n_packets, const int32_t* d_seq_base, int32_t first_seq, solo_arrival_t* d_records,
                         int32_t max_records, uint8_t* d_payload, int64_t payload_capacity, solo_send_count_t* d_count, void* hip_stream) {
    if (!b || !sx_fan_args_ok(d_bits, d_nbytes, n_src, d_source, n_dst, n_packets, d_records, max_records, d_payload, payload_capacity, d_count)) return -1;
    hipStream_t st = (hipStream_t)hip_stream;
    SOLO_CHECK(grow_scratch(b->d_send_scratch, b->send_scratch_bytes, solo_fan_scratch_bytes(n_src, n_dst, n_packets), st));
    SxFanArgs a;
    a.bits = d_bits; a.nbytes = d_nbytes; a.source = d_source; a.dst_stream = d_dst_stream; a.send = d_send; a.seq_base = d_seq_base;
    a.named = NULL; a.pool_off = NULL;
    a.n_src = n_src; a.n_dst = n_dst; a.n_packets = n_packets; a.slot = b->slot; a.first_seq = first_seq;
    a.hbb = handle_hb_bytes(b);
    SOLO_CHECK(solo_fan_launch(a, b->d_send_scratch, d_records, max_records, d_payload, (long long)payload_capacity, d_count, b->d_verdict + SOLO_VERDICT_SEND, st));
    return 0;
}

// ---- mixing bridge (solo_mix.h): decoded rows -> mix-minus rows, room by room ------------------------------------------------------
int32_t solo_mix(solo_batch_t* b, const int16_t* d_pcm_in, int32_t n, int32_t n_packets, const int32_t* d_room, int32_t n_rooms,
                 const int16_t* d_gain_q12, int32_t max_speakers, int16_t* d_pcm_out, int64_t* d_energy, uint8_t* d_mixed, solo_mix_count_t* d_count,
                 void* hip_stream) {
    if (!b || !d_pcm_in || !d_room || !d_pcm_out || n <= 0 || n_packets <= 0 || n_rooms <= 0 || n_rooms > n) return -1;
    if ((int64_t)n * (int64_t)n_packets >= ((int64_t)1 << 31)) return -1;
    if (max_speakers > SX_MIX_MAX_SPEAKERS || (max_speakers <= 0 && n > SX_MIX_MAX_ALL_ROWS)) return -1;
    const int L = handle_packet_samples(b);
    if (L <= 0 || L > SX_MIX_MAX_L || (L & 7)) return -1;
    const uintptr_t in0 = (uintptr_t)d_pcm_in, out0 = (uintptr_t)d_pcm_out;
    const uintptr_t bytes = (uintptr_t)n * (uintptr_t)n_packets * (uintptr_t)L * sizeof(int16_t);
    if ((in0 & 15) || (out0 & 15) || (in0 < out0 + bytes && out0 < in0 + bytes)) return -1;
    hipStream_t st = (hipStream_t)hip_stream;
    SOLO_CHECK(grow_scratch(b->d_mix_scratch, b->mix_scratch_bytes, solo_mix_scratch_bytes(n, n_packets), st));
    SxMixArgs a;
    a.pcm_in = d_pcm_in; a.gain = d_gain_q12; a.pcm_out = d_pcm_out; a.energy = d_energy; a.mixed = d_mixed;
    a.counts = NULL; a.starts = NULL; a.members = NULL;
    a.n_packets = n_packets; a.L = L; a.max_speakers = max_speakers;
    SOLO_CHECK(solo_mix_launch(a, d_room, n, n_rooms, b->d_mix_scratch, d_count, b->d_verdict + SOLO_VERDICT_MIX, st));
    return 0;
}

// ... with shared listener mixes (solo_mix_shared.h): a personal row per speaker, one row per room for everybody else
int32_t solo_mix_shared(solo_batch_t* b, const int16_t* d_pcm_in, int32_t n, int32_t n_packets, const int32_t* d_room, int32_t n_rooms,
                        const int16_t* d_gain_q12, int32_t max_speakers, const uint8_t* d_keep, const int32_t* d_slots, int16_t* d_pcm_spk,
                        int32_t* d_spk_list, int32_t* d_spk_rows, int16_t* d_pcm_room, int32_t* d_room_list, int32_t* d_source, int64_t* d_energy,
                        uint8_t* d_mixed, solo_mix_shared_count_t* d_count, void* hip_stream) {
    if (!b) return -1;
    const int L = handle_packet_samples(b);
    if (!sx_mixsh_args_ok(d_pcm_in, n, n_packets, L, d_room, n_rooms, max_speakers, d_pcm_spk, d_spk_list, d_pcm_room, d_room_list, d_source, d_count)) return -1;
    hipStream_t st = (hipStream_t)hip_stream;
    SOLO_CHECK(grow_scratch(b->d_mix_scratch, b->mix_scratch_bytes, solo_mixsh_scratch_bytes(n, n_packets), st));
    SxMixShArgs a = {};
    a.pcm_in = d_pcm_in; a.gain = d_gain_q12; a.room = d_room; a.keep = d_keep; a.slots = d_slots;
    a.pcm_spk = d_pcm_spk; a.spk_list = d_spk_list; a.spk_rows = d_spk_rows; a.pcm_room = d_pcm_room; a.room_list = d_room_list; a.source = d_source;
    a.energy = d_energy; a.mixed = d_mixed;
    a.n = n; a.n_rooms = n_rooms; a.n_packets = n_packets; a.L = L; a.max_speakers = max_speakers;
    SOLO_CHECK(solo_mixsh_launch(a, b->d_mix_scratch, d_count, b->d_verdict + SOLO_VERDICT_MIX, st));
    return 0;
}

// ... from a selection the caller brings (solo_mix_selected.h): no energies, no select pass
int32_t solo_mix_selected(solo_batch_t* b, const int16_t* d_pcm_in, int32_t n, int32_t n_packets, const int32_t* d_room, int32_t n_rooms,
                          const int16_t* d_gain_q12, const uint8_t* d_sel, const uint8_t* d_keep, const int32_t* d_slots, int16_t* d_pcm_spk,
                          int32_t* d_spk_list, int32_t* d_spk_rows, int16_t* d_pcm_room, int32_t* d_room_list, int32_t* d_source,
                          uint8_t* d_room_nsel, int64_t* d_energy, solo_mix_selected_count_t* d_count, void* hip_stream) {
    if (!b) return -1;
    const int L = handle_packet_samples(b);
    if (!sx_mixsel_args_ok(d_pcm_in, n, n_packets, L, d_room, n_rooms, d_sel, d_pcm_spk, d_spk_list, d_pcm_room, d_room_list, d_source, d_count)) return -1;
    hipStream_t st = (hipStream_t)hip_stream;
    SOLO_CHECK(grow_scratch(b->d_mix_scratch, b->mix_scratch_bytes, solo_mixsel_scratch_bytes(n, n_packets), st));
    SxMixSelArgs a = {};
    a.sh.pcm_in = d_pcm_in; a.sh.gain = d_gain_q12; a.sh.room = d_room; a.sh.keep = d_keep; a.sh.slots = d_slots;
    a.sh.pcm_spk = d_pcm_spk; a.sh.spk_list = d_spk_list; a.sh.spk_rows = d_spk_rows; a.sh.pcm_room = d_pcm_room; a.sh.room_list = d_room_list;
    a.sh.source = d_source; a.sh.energy = d_energy; a.sh.mixed = const_cast<uint8_t*>(d_sel);       // (read only on this path)
    a.sh.n = n; a.sh.n_rooms = n_rooms; a.sh.n_packets = n_packets; a.sh.L = L; a.sh.max_speakers = SX_MIX_MAX_SPEAKERS;
    a.room_nsel = d_room_nsel;
    SOLO_CHECK(solo_mixsel_launch(a, b->d_mix_scratch, d_count, b->d_verdict + SOLO_VERDICT_MIX, st));
    return 0;
}

// ---- play-out time scaling (solo_timescale.h): in_packets decoded packets of a row -> out_packets packets of audio ---------------------
int32_t solo_timescale(solo_batch_t* b, const int16_t* d_pcm_in, int32_t n, int32_t in_packets, int32_t out_packets, int16_t* d_pcm_out,
                       int32_t* d_shift, int32_t* d_cost, solo_timescale_count_t* d_count, void* hip_stream) {
    if (!b) return -1;
    int fs;
    const int L = handle_packet_samples(b, &fs);
    if (!sx_ts_args_ok(d_pcm_in, n, in_packets, out_packets, fs, L, d_pcm_out)) return -1;
    SxTsArgs a;
    a.pcm_in = d_pcm_in; a.pcm_out = d_pcm_out; a.shift = d_shift; a.cost = d_cost;
    a.Li = in_packets * L; a.Lo = out_packets * L; a.H = fs / 200;
    SOLO_CHECK(solo_timescale_launch(a, n, d_count, (hipStream_t)hip_stream));
    return 0;
}

// ---- the row-state objects: Resampler, Vad, Agc, Rate, Playout ------------------------------------------------------------------------------
// Each sits beside a handle, holds one state record per row, carries it from call to call and derives from solo_rows; what is written
// here once is their whole lifecycle (solo_rows.h has the kernels).  The entry points keep their own argument checks.
struct solo_rows {
    int32_t n_rows, words;           // rows; 32-bit words of a row's state record
    int32_t* d_state;                // [n_rows][words]
    uint32_t* d_verdict;             // the verdict words of the object's calls (launch_list_check)
    int32_t* d_extra;                // [n_rows][extra_words]: a row's second segment (Playout's held packet), or NULL
    int32_t extra_words;
    SxRowInit init;                  // the record a reset leaves
};
static void rows_free(solo_rows* o) {
    dev_free(o->d_state);
    dev_free(o->d_verdict);
    dev_free(o->d_extra);
}
static int32_t rows_reset(solo_rows* o, hipStream_t st) {
    if (!o) return -1;
    const size_t words = (size_t)o->n_rows * ((size_t)o->words + (size_t)o->extra_words);
    hipLaunchKernelGGL(solo_rows_reset_all_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st, o->d_state, o->words, o->init, o->d_extra, o->extra_words,
                       o->n_rows);
    SOLO_CHECK(hipGetLastError());
    return 0;
}
// h_rows: a HOST list (sx_list_ok); it travels by value, SX_CTL_PER_LAUNCH rows a launch
static int32_t rows_reset_list(solo_rows* o, const int32_t* h_rows, int32_t n, hipStream_t st) {
    if (!o || !sx_list_ok(h_rows, n, o->n_rows)) return -1;
    std::vector<SxStreamCtl> recs((size_t)n);
    for (int32_t i = 0; i < n; i++) recs[i] = SxStreamCtl{h_rows[i], 0, 0, 0};
    SOLO_CHECK(sx_launch_ctl_batches(recs.data(), n, [&](const SxStreamCtlList& l, int k) {
        hipLaunchKernelGGL(solo_rows_reset_kernel, dim3((unsigned)k), dim3(64), 0, st, o->d_state, o->words, o->init, o->d_extra, o->extra_words, l);
    }));
    return 0;
}
// the get_state (put = 0) and set_state calls: d_rows on the device, NULL = rows 0 .. n - 1; an index outside [0, n_rows) moves nothing
static int32_t rows_copy_state(solo_rows* o, const int32_t* d_rows, int32_t n, uint8_t* d_blob, int put, hipStream_t st) {
    if (!o || !d_blob || n <= 0 || n > o->n_rows || ((uintptr_t)d_blob & 3)) return -1;
    const size_t words = (size_t)n * ((size_t)o->words + (size_t)o->extra_words);
    hipLaunchKernelGGL(solo_rows_copy_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st, o->d_state, o->words, o->d_extra, o->extra_words, o->n_rows,
                       d_rows, n, (i32*)d_blob, put);
    SOLO_CHECK(hipGetLastError());
    return 0;
}
// the create calls: the records (init_word(w): word w of the initial record, NULL: zeros), n_verdicts verdict words and the second
// segment, all as a reset leaves them.  The create call's last step: it ends with the synchronisation that the caller's own memsets
// need as well.  false: the caller's destroy call frees what there is (rows_free)
static bool rows_alloc(solo_rows* o, int32_t n_rows, int32_t words, i32 (*init_word)(int), int32_t n_verdicts, int32_t extra_words) {
    o->n_rows = n_rows; o->words = words; o->extra_words = extra_words;
    for (int w = 0; w < words; w++) o->init.w[w] = init_word ? init_word(w) : 0;
    return hipMalloc((void**)&o->d_state, (size_t)n_rows * words * sizeof(int32_t)) == hipSuccess &&
           hipMalloc((void**)&o->d_verdict, n_verdicts * sizeof(uint32_t)) == hipSuccess && hipMemset(o->d_verdict, 0, n_verdicts * sizeof(uint32_t)) == hipSuccess &&
           (!extra_words || hipMalloc((void**)&o->d_extra, (size_t)n_rows * extra_words * sizeof(int32_t)) == hipSuccess) && rows_reset(o, NULL) == 0 &&
           hipStreamSynchronize(NULL) == hipSuccess;
}

// ---- PCM rate conversion (solo_resample.h): it sits between two handles of different rates; a zeroed record = SKP_Silk_resampler_init ----
static_assert(SX_RS_STATE_WORDS <= SX_ROWS_MAX_WORDS, "solo_resample.h and solo_rows.h agree");
struct solo_resampler : solo_rows {
    int32_t fs_in, fs_out;
    SxRsCfg cfg;
};
solo_resampler_t* solo_resample_create(int32_t n_rows, int32_t fs_in, int32_t fs_out) {
    SxRsCfg cfg;
    if (n_rows <= 0 || !sx_rs_config(fs_in, fs_out, &cfg) || !have_device()) return NULL;
    solo_resampler* r = new (std::nothrow) solo_resampler();
    if (!r) return NULL;
    r->fs_in = fs_in; r->fs_out = fs_out; r->cfg = cfg;
    if (!rows_alloc(r, n_rows, SX_RS_STATE_WORDS, NULL, 1, 0)) {
        solo_resample_destroy(r);
        return NULL;
    }
    return r;
}
void solo_resample_destroy(solo_resampler_t* r) {
    if (!r) return;
    rows_free(r);
    delete r;
}
int32_t solo_resample_out_samples(const solo_resampler_t* r, int32_t in_samples) { return r ? sx_rs_out_samples(r->cfg, in_samples) : -1; }
int32_t solo_resample_reset(solo_resampler_t* r, void* hip_stream) { return rows_reset(r, (hipStream_t)hip_stream); }
int32_t solo_resample_reset_rows(solo_resampler_t* r, const int32_t* h_rows, int32_t n, void* hip_stream) {
    return rows_reset_list(r, h_rows, n, (hipStream_t)hip_stream);
}
static int32_t resample_call(solo_resampler* r, const int32_t* d_rows, int32_t n, const int16_t* d_in, int32_t n_packets, int32_t in_samples,
                             int16_t* d_out, solo_resample_count_t* d_count, hipStream_t st) {
    if (!sx_rs_call_ok(r->cfg, r->n_rows, n, n_packets, in_samples, d_in, d_out)) return -1;
    SxRsArgs a;
    a.c = r->cfg; a.in = d_in; a.out = d_out; a.state = r->d_state; a.map = d_rows; a.n = n;
    a.batches = n_packets * (in_samples / r->cfg.n_in);
    SOLO_CHECK(launch_list_check(d_rows, n, r->n_rows, r->d_verdict, NULL, st));
    SOLO_CHECK(solo_resample_launch(a, d_count, r->d_verdict, st));
    return 0;
}
int32_t solo_resample(solo_resampler_t* r, const int16_t* d_in, int32_t n_packets, int32_t in_samples, int16_t* d_out, void* hip_stream) {
    if (!r) return -1;
    return resample_call(r, NULL, r->n_rows, d_in, n_packets, in_samples, d_out, NULL, (hipStream_t)hip_stream);
}
int32_t solo_resample_rows(solo_resampler_t* r, const int32_t* d_rows, int32_t n, const int16_t* d_in, int32_t n_packets, int32_t in_samples,
                           int16_t* d_out, solo_resample_count_t* d_count, void* hip_stream) {
    if (!r || !d_rows || !d_count) return -1;
    return resample_call(r, d_rows, n, d_in, n_packets, in_samples, d_out, d_count, (hipStream_t)hip_stream);
}

// ---- voice activity, audio level, speaker selection (solo_vad.h): an object of its own, with a state record per row -------------------
static_assert(SOLO_VAD_STATE_BYTES == SX_VAD_STATE_WORDS * 4 && SX_VAD_STATE_WORDS <= SX_ROWS_MAX_WORDS, "include/solo_mi355x.h, solo_vad.h and solo_rows.h agree");
struct solo_vad_obj : solo_rows {    // d_verdict[2]: the verdict words of solo_vad and of solo_vad_select
    int32_t frame;
    void* d_scratch;                 // the room plan and the keys of solo_vad_select (solo_vad_scratch_bytes)
};
solo_vad_t* solo_vad_create(int32_t n_rows, int32_t frame_samples) {
    if (n_rows <= 0 || !sx_vad_frame_ok(frame_samples) || (int64_t)n_rows * SX_VAD_STATE_WORDS >= ((int64_t)1 << 31) || !have_device()) return NULL;
    solo_vad_obj* v = new (std::nothrow) solo_vad_obj();
    if (!v) return NULL;
    v->frame = frame_samples;
    if (hipMalloc(&v->d_scratch, solo_vad_scratch_bytes(n_rows)) != hipSuccess || !rows_alloc(v, n_rows, SX_VAD_STATE_WORDS, sx_vad_init_word, 2, 0)) {
        solo_vad_destroy(v);
        return NULL;
    }
    return v;
}
void solo_vad_destroy(solo_vad_t* v) {
    if (!v) return;
    rows_free(v);
    dev_free(v->d_scratch);
    delete v;
}
int32_t solo_vad_reset(solo_vad_t* v, void* hip_stream) { return rows_reset(v, (hipStream_t)hip_stream); }
int32_t solo_vad_reset_rows(solo_vad_t* v, const int32_t* h_rows, int32_t n, void* hip_stream) { return rows_reset_list(v, h_rows, n, (hipStream_t)hip_stream); }
int32_t solo_vad_get_state(solo_vad_t* v, const int32_t* d_rows, int32_t n, uint8_t* d_blob, void* hip_stream) {
    return rows_copy_state(v, d_rows, n, d_blob, 0, (hipStream_t)hip_stream);
}
int32_t solo_vad_set_state(solo_vad_t* v, const int32_t* d_rows, int32_t n, const uint8_t* d_blob, void* hip_stream) {
    return rows_copy_state(v, d_rows, n, (uint8_t*)d_blob, 1, (hipStream_t)hip_stream);
}
int32_t solo_vad(solo_vad_t* v, const int32_t* d_rows, int32_t n, const int16_t* d_pcm, int32_t n_packets, int32_t packet_samples, uint8_t* d_sa_q8,
                 int32_t* d_detail, uint8_t* d_level, solo_vad_count_t* d_count, void* hip_stream) {
    if (!v || !sx_vad_call_ok(v->frame, v->n_rows, d_rows, n, d_pcm, n_packets, packet_samples, d_sa_q8, d_count)) return -1;
    hipStream_t st = (hipStream_t)hip_stream;
    SxVadArgs a;
    a.pcm = d_pcm; a.state = v->d_state; a.map = d_rows; a.sa = d_sa_q8; a.detail = d_detail; a.level = d_level;
    a.n = n; a.n_packets = n_packets; a.packet_samples = packet_samples;
    SOLO_CHECK(launch_list_check(d_rows, n, v->n_rows, v->d_verdict, NULL, st));
    SOLO_CHECK(solo_vad_launch(v->frame, a, d_count, v->d_verdict, st));
    return 0;
}
int32_t solo_vad_select(solo_vad_t* v, const int32_t* d_rows, int32_t n, const uint8_t* d_sa_q8, const uint8_t* d_level, int32_t n_packets, int32_t frames,
                        const int32_t* d_room, int32_t n_rooms, const solo_vad_select_params_t* params, const int16_t* d_gain_in, uint8_t* d_sel,
                        int16_t* d_gain_out, uint8_t* d_keep, int32_t* d_dominant, solo_vad_count_t* d_count, void* hip_stream) {
    if (!v || !sx_vsel_call_ok(v->n_rows, n, d_sa_q8, d_level, n_packets, frames, d_room, n_rooms, params, d_sel, d_count)) return -1;
    hipStream_t st = (hipStream_t)hip_stream;
    SxVselArgs a = {};
    a.sa = d_sa_q8; a.level = d_level; a.gain_in = d_gain_in; a.map = d_rows;
    a.sel = d_sel; a.gain_out = d_gain_out; a.keep = d_keep; a.dominant = d_dominant; a.state = v->d_state;
    a.n_packets = n_packets; a.frames = frames; a.prm = *params;
    const int32_t n_rows = v->n_rows;
    hipError_t lerr = hipSuccess;
    SOLO_CHECK(solo_vad_select_launch(a, d_room, n, n_rooms, n_rows, v->d_scratch, d_count, v->d_verdict + 1, [&](u32* verdict) {
        lerr = launch_list_check(d_rows, n, n_rows, verdict, NULL, st);
    }, st));
    SOLO_CHECK(lerr);
    return 0;
}

// ---- level control and peak limiter (solo_agc.h): an object of its own, with a state record per row -----------------------------------
static_assert(SOLO_AGC_STATE_BYTES == SX_AGC_STATE_WORDS * 4 && SX_AGC_STATE_WORDS <= SX_ROWS_MAX_WORDS, "include/solo_mi355x.h, solo_agc.h and solo_rows.h agree");
struct solo_agc_obj : solo_rows {
    unsigned long long* d_acc;       // the counters of a call's count (solo_agc_acc_bytes; zero between calls)
};
solo_agc_t* solo_agc_create(int32_t n_rows) {
    if (n_rows <= 0 || (int64_t)n_rows * SX_AGC_STATE_WORDS >= ((int64_t)1 << 31) || !have_device()) return NULL;
    solo_agc_obj* g = new (std::nothrow) solo_agc_obj();
    if (!g) return NULL;
    if (hipMalloc((void**)&g->d_acc, solo_agc_acc_bytes(n_rows)) != hipSuccess || hipMemset(g->d_acc, 0, solo_agc_acc_bytes(n_rows)) != hipSuccess ||
        !rows_alloc(g, n_rows, SX_AGC_STATE_WORDS, sx_agc_init_word, 1, 0)) {
        solo_agc_destroy(g);
        return NULL;
    }
    return g;
}
void solo_agc_destroy(solo_agc_t* g) {
    if (!g) return;
    rows_free(g);
    dev_free(g->d_acc);
    delete g;
}
int32_t solo_agc_reset(solo_agc_t* g, void* hip_stream) { return rows_reset(g, (hipStream_t)hip_stream); }
int32_t solo_agc_reset_rows(solo_agc_t* g, const int32_t* h_rows, int32_t n, void* hip_stream) { return rows_reset_list(g, h_rows, n, (hipStream_t)hip_stream); }
int32_t solo_agc_get_state(solo_agc_t* g, const int32_t* d_rows, int32_t n, uint8_t* d_blob, void* hip_stream) {
    return rows_copy_state(g, d_rows, n, d_blob, 0, (hipStream_t)hip_stream);
}
int32_t solo_agc_set_state(solo_agc_t* g, const int32_t* d_rows, int32_t n, const uint8_t* d_blob, void* hip_stream) {
    return rows_copy_state(g, d_rows, n, (uint8_t*)d_blob, 1, (hipStream_t)hip_stream);
}
int32_t solo_agc(solo_agc_t* g, const int32_t* d_rows, int32_t n, const int16_t* d_pcm_in, int32_t n_packets, int32_t packet_samples,
                 const uint8_t* d_level_in, const uint8_t* d_sa_q8, int32_t frames, const solo_agc_params_t* params, int16_t* d_pcm_out,
                 uint8_t* d_level_out, int16_t* d_gain_q8, solo_agc_count_t* d_count, void* hip_stream) {
    if (!g || !sx_agc_call_ok(g->n_rows, d_rows, n, d_pcm_in, n_packets, packet_samples, d_sa_q8, frames, params, d_pcm_out, d_count))
        return -1;
    hipStream_t st = (hipStream_t)hip_stream;
    SxAgcArgs a;
    a.in = d_pcm_in; a.out = d_pcm_out; a.state = g->d_state; a.map = d_rows; a.level_in = d_level_in; a.sa = d_sa_q8;
    a.level_out = d_level_out; a.gain_out = d_gain_q8;
    a.n = n; a.n_packets = n_packets; a.packet_samples = packet_samples; a.frames = d_sa_q8 ? frames : 0; a.prm = *params;
    SOLO_CHECK(launch_list_check(d_rows, n, g->n_rows, g->d_verdict, NULL, st));
    SOLO_CHECK(solo_agc_launch(a, d_count, g->d_acc, g->d_verdict, st));
    return 0;
}

// ---- the sender's rate controller (solo_rate.h): an object of its own, with a state record per row; the send mask is stateless ---------
static_assert(SOLO_RATE_STATE_BYTES == SX_RATE_STATE_WORDS * 4 && SX_RATE_STATE_WORDS <= SX_ROWS_MAX_WORDS, "include/solo_mi355x.h, solo_rate.h and solo_rows.h agree");
struct solo_rate_obj : solo_rows {};
solo_rate_t* solo_rate_create(int32_t n_rows) {
    if (n_rows <= 0 || (int64_t)n_rows * SX_RATE_STATE_WORDS >= ((int64_t)1 << 31) || !have_device()) return NULL;
    solo_rate_obj* rc = new (std::nothrow) solo_rate_obj();
    if (!rc) return NULL;
    if (!rows_alloc(rc, n_rows, SX_RATE_STATE_WORDS, sx_rate_init_word, 1, 0)) {
        solo_rate_destroy(rc);
        return NULL;
    }
    return rc;
}
void solo_rate_destroy(solo_rate_t* rc) {
    if (!rc) return;
    rows_free(rc);
    delete rc;
}
int32_t solo_rate_reset(solo_rate_t* rc, void* hip_stream) { return rows_reset(rc, (hipStream_t)hip_stream); }
int32_t solo_rate_reset_rows(solo_rate_t* rc, const int32_t* h_rows, int32_t n, void* hip_stream) { return rows_reset_list(rc, h_rows, n, (hipStream_t)hip_stream); }
int32_t solo_rate_get_state(solo_rate_t* rc, const int32_t* d_rows, int32_t n, uint8_t* d_blob, void* hip_stream) {
    return rows_copy_state(rc, d_rows, n, d_blob, 0, (hipStream_t)hip_stream);
}
int32_t solo_rate_set_state(solo_rate_t* rc, const int32_t* d_rows, int32_t n, const uint8_t* d_blob, void* hip_stream) {
    return rows_copy_state(rc, d_rows, n, (uint8_t*)d_blob, 1, (hipStream_t)hip_stream);
}
int32_t solo_rate_update(solo_rate_t* rc, const solo_rtcp_feedback_t* d_feedback, const solo_rate_params_t* params, int32_t* d_target_bps, uint8_t* d_mode,
                         solo_rate_count_t* d_count, void* hip_stream) {
    if (!rc || !sx_rate_update_call_ok(rc->n_rows, d_feedback, params, d_target_bps, d_mode, d_count)) return -1;
    SxRateArgs a;
    a.feedback = (const u32*)d_feedback; a.state = rc->d_state; a.target = d_target_bps; a.mode = d_mode; a.count = (i32*)d_count;
    a.p = *params; a.n_rows = rc->n_rows;
    SOLO_CHECK(solo_rate_update_launch(a, (hipStream_t)hip_stream));
    return 0;
}
int32_t solo_rate_send_mask(const uint8_t* d_mode, int32_t n_rows, const int32_t* d_streams, int32_t n, int32_t n_packets, const int32_t* d_seq_base,
                            int32_t first_seq, const uint8_t* d_send_in, uint8_t* d_send, void* hip_stream) {
    if (!sx_rate_mask_call_ok(d_mode, n_rows, d_streams, n, n_packets, d_seq_base, d_send)) return -1;
    SxRateMaskArgs a;
    a.mode = d_mode; a.map = d_streams; a.seq_base = d_seq_base; a.send_in = d_send_in; a.send = d_send;
    a.n_rows = n_rows; a.n = n; a.n_packets = n_packets; a.first_seq = first_seq;
    SOLO_CHECK(solo_rate_send_mask_launch(a, (hipStream_t)hip_stream));
    return 0;
}

// ---- adaptive play-out delay control (solo_playout.h): an object of its own, a state record and a held packet per row ------------------
static_assert(SOLO_PLAYOUT_STATE_BYTES == SX_PO_STATE_WORDS * 4 && SX_PO_STATE_WORDS <= SX_ROWS_MAX_WORDS, "include/solo_mi355x.h, solo_playout.h and solo_rows.h agree");
struct solo_playout_obj : solo_rows {    // d_verdict[2]: the verdict words of the plan and of the render; d_extra: the held packets, int16 [n_rows][L]
    int32_t L;
    int32_t *d_slot, *d_sslot;       // [n_rows]: where the last plan put each row (solo_playout_compact_kernel)
    // the tick's intermediates, one allocation (d_scratch) cut up at create
    void* d_scratch;
    uint32_t* d_reports;
    int32_t *d_action, *d_one, *d_two, *d_spos, *d_st_one, *d_st_two, *d_cost_s, *d_cost_a;
    int16_t *d_pcm_one, *d_pcm_two, *d_gath, *d_ts_s, *d_ts_a;
    SxPoPlanCount* h_count;          // pinned: where the tick reads the plan count
};
solo_playout_t* solo_playout_create(int32_t n_rows, int32_t packet_samples) {
    if (!sx_po_geometry_ok(n_rows, packet_samples) || !have_device()) return NULL;
    solo_playout_obj* po = new (std::nothrow) solo_playout_obj();
    if (!po) return NULL;
    po->L = packet_samples;
    const size_t n = (size_t)n_rows, L = (size_t)packet_samples;
    size_t off = 0;
    auto cut = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_rep = cut(n * 64), o_act = cut(n * 4), o_one = cut(n * 4), o_two = cut(n * 4), o_spos = cut(n * 4), o_st1 = cut(n * 4), o_st2 = cut(n * 4),
                 o_cs = cut(n * 2 * SX_TS_MAX_BLOCKS * 2), o_ca = cut(n * SX_TS_MAX_BLOCKS * 2), o_p1 = cut(n * L * 2), o_p2 = cut(n * L * 4), o_g = cut(n * L * 2),
                 o_ts = cut(n * L * 4), o_ta = cut(n * L * 2);
    if (hipMalloc((void**)&po->d_slot, n * sizeof(int32_t)) != hipSuccess || hipMalloc((void**)&po->d_sslot, n * sizeof(int32_t)) != hipSuccess ||
        hipMalloc(&po->d_scratch, off) != hipSuccess || hipHostMalloc((void**)&po->h_count, sizeof(SxPoPlanCount)) != hipSuccess ||
        hipMemset(po->d_slot, 0xFF, n * sizeof(int32_t)) != hipSuccess || hipMemset(po->d_sslot, 0xFF, n * sizeof(int32_t)) != hipSuccess ||
        !rows_alloc(po, n_rows, SX_PO_STATE_WORDS, NULL, 2, packet_samples / 2)) {
        solo_playout_destroy(po);
        return NULL;
    }
    char* base = (char*)po->d_scratch;
    po->d_reports = (uint32_t*)(base + o_rep); po->d_action = (int32_t*)(base + o_act); po->d_one = (int32_t*)(base + o_one); po->d_two = (int32_t*)(base + o_two);
    po->d_spos = (int32_t*)(base + o_spos); po->d_st_one = (int32_t*)(base + o_st1); po->d_st_two = (int32_t*)(base + o_st2);
    po->d_cost_s = (int32_t*)(base + o_cs); po->d_cost_a = (int32_t*)(base + o_ca); po->d_pcm_one = (int16_t*)(base + o_p1); po->d_pcm_two = (int16_t*)(base + o_p2);
    po->d_gath = (int16_t*)(base + o_g); po->d_ts_s = (int16_t*)(base + o_ts); po->d_ts_a = (int16_t*)(base + o_ta);
    return po;
}
void solo_playout_destroy(solo_playout_t* po) {
    if (!po) return;
    rows_free(po);
    dev_free(po->d_slot);
    dev_free(po->d_sslot);
    dev_free(po->d_scratch);
    if (po->h_count) (void)hipHostFree(po->h_count);
    delete po;
}
int32_t solo_playout_reset(solo_playout_t* po, void* hip_stream) { return rows_reset(po, (hipStream_t)hip_stream); }
int32_t solo_playout_reset_rows(solo_playout_t* po, const int32_t* h_rows, int32_t n, void* hip_stream) {
    return rows_reset_list(po, h_rows, n, (hipStream_t)hip_stream);
}
int32_t solo_playout_get_state(solo_playout_t* po, const int32_t* d_rows, int32_t n, uint8_t* d_blob, void* hip_stream) {
    return rows_copy_state(po, d_rows, n, d_blob, 0, (hipStream_t)hip_stream);
}
int32_t solo_playout_set_state(solo_playout_t* po, const int32_t* d_rows, int32_t n, const uint8_t* d_blob, void* hip_stream) {
    return rows_copy_state(po, d_rows, n, (uint8_t*)d_blob, 1, (hipStream_t)hip_stream);
}
int32_t solo_playout_plan(solo_playout_t* po, const solo_recv_report_t* d_reports, const int32_t* d_rows, int32_t n, int32_t depth,
                          const solo_playout_params_t* params, int32_t* d_action, int32_t* d_one, int32_t* d_two, int32_t* d_stretch_pos,
                          solo_playout_plan_count_t* d_count, void* hip_stream) {
    if (!po || !sx_po_plan_call_ok(po->n_rows, d_reports, d_rows, n, depth, params, d_action, d_one, d_two, d_stretch_pos, d_count)) return -1;
    hipStream_t st = (hipStream_t)hip_stream;
    SOLO_CHECK(launch_list_check(d_rows, n, po->n_rows, po->d_verdict, NULL, st));
    SxPoPlanArgs a;
    a.reports = (const uint32_t*)d_reports; a.state = po->d_state; a.map = d_rows; a.action = d_action; a.p = *params; a.n = n; a.depth = depth;
    SOLO_CHECK(solo_playout_plan_launch(a, d_one, d_two, d_stretch_pos, po->d_slot, po->d_sslot, (SxPoPlanCount*)d_count, po->d_verdict, st));
    return 0;
}
int32_t solo_playout_gather(solo_playout_t* po, const int16_t* d_pcm_one, int32_t n_one, const int32_t* d_stretch_pos, int32_t n_stretch, int16_t* d_out,
                            void* hip_stream) {
    if (!po || !sx_po_gather_call_ok(po->n_rows, d_pcm_one, n_one, d_stretch_pos, n_stretch, d_out)) return -1;
    SOLO_CHECK(solo_playout_gather_launch(d_pcm_one, d_stretch_pos, n_one, n_stretch, po->L, d_out, (hipStream_t)hip_stream));
    return 0;
}
int32_t solo_playout_render(solo_playout_t* po, const int32_t* d_rows, int32_t n, const solo_playout_params_t* params, int32_t block_samples,
                            const int32_t* d_action, int32_t n_one, int32_t n_two, int32_t n_stretch, const int16_t* d_pcm_one, const int32_t* d_status_one,
                            const int16_t* d_pcm_two, const int32_t* d_status_two, const int16_t* d_ts_stretch, const int32_t* d_cost_stretch,
                            const int16_t* d_ts_accel, const int32_t* d_cost_accel, int16_t* d_heard, int32_t* d_outcome, int32_t* d_status,
                            solo_playout_render_count_t* d_count, void* hip_stream) {
    if (!po || !sx_po_render_call_ok(po->n_rows, po->L, d_rows, n, params, block_samples, d_action, n_one, n_two, n_stretch, d_pcm_one,
                                     d_status_one, d_pcm_two, d_status_two, d_ts_stretch, d_cost_stretch, d_ts_accel, d_cost_accel, d_heard, d_outcome, d_status, d_count))
        return -1;
    hipStream_t st = (hipStream_t)hip_stream;
    SOLO_CHECK(launch_list_check(d_rows, n, po->n_rows, po->d_verdict + 1, NULL, st));
    SxPoRenderArgs a;
    a.state = po->d_state; a.held = (int16_t*)po->d_extra; a.map = d_rows; a.action = d_action; a.slot = po->d_slot; a.sslot = po->d_sslot;
    a.pcm_one = d_pcm_one; a.st_one = d_status_one; a.pcm_two = d_pcm_two; a.st_two = d_status_two; a.ts_s = d_ts_stretch; a.cost_s = d_cost_stretch;
    a.ts_a = d_ts_accel; a.cost_a = d_cost_accel; a.heard = d_heard; a.outcome = d_outcome; a.status = d_status;
    a.n = n; a.n_one = n_one; a.n_two = n_two; a.n_stretch = n_stretch; a.L = po->L; a.M = po->L / block_samples;
    a.cooldown = params->cooldown; a.cost_gate = params->cost_gate;
    SOLO_CHECK(solo_playout_render_launch(a, (SxPoRenderCount*)d_count, po->d_verdict + 1, st));
    return 0;
}
int32_t solo_playout_tick(solo_playout_t* po, solo_batch_t* b, const int32_t* d_streams, int32_t n, const solo_playout_params_t* params, int16_t* d_heard,
                          int32_t* d_outcome, int32_t* d_status, solo_playout_count_t* d_count, void* hip_stream) {
    if (!po || !b) return -1;
    int fs = 0;
    const int L = handle_packet_samples(b, &fs), H = fs / 200;
    if (!sx_po_tick_call_ok(po->n_rows, po->L, b->d_recv_ring != NULL, b->recv_track != 0, b->n_streams, b->recv_depth, L, fs, d_streams, n, params,
                            d_heard, d_outcome, d_status, d_count))
        return -1;
    hipStream_t st = (hipStream_t)hip_stream;
    int32_t r = solo_recv_report(b, d_streams, n, NULL, 0, 0, SOLO_RECV_REPORT_CLEAR_MARGIN, (solo_recv_report_t*)po->d_reports, NULL, NULL, NULL, hip_stream);
    if (r) return r;
    if ((r = solo_playout_plan(po, (const solo_recv_report_t*)po->d_reports, d_streams, n, b->recv_depth, params, po->d_action, po->d_one, po->d_two, po->d_spos,
                               &d_count->plan, hip_stream)) != 0)
        return r;
    // the tick's one synchronisation: how many rows each of the calls below gets
    SOLO_CHECK(hipMemcpyAsync(po->h_count, &d_count->plan, sizeof(SxPoPlanCount), hipMemcpyDeviceToHost, st));
    SOLO_CHECK(hipStreamSynchronize(st));
    const SxPoPlanCount c = *po->h_count;
    if (c.n_one < 0) return 0;                               // (the list was refused on the device: d_count->plan.n_one = -1 says so, nothing else is written)
    if (c.n_one > n || c.n_two < 0 || c.n_two > n || c.n_stretch < 0 || c.n_stretch > c.n_one) return -1;
    if (c.n_one && (r = solo_recv_decode_streams(b, po->d_one, c.n_one, 1, po->d_pcm_one, po->d_st_one, hip_stream)) != 0) return r;
    if (c.n_two && (r = solo_recv_decode_streams(b, po->d_two, c.n_two, 2, po->d_pcm_two, po->d_st_two, hip_stream)) != 0) return r;
    if (c.n_stretch) {
        if ((r = solo_playout_gather(po, po->d_pcm_one, c.n_one, po->d_spos, c.n_stretch, po->d_gath, hip_stream)) != 0) return r;
        if ((r = solo_timescale(b, po->d_gath, c.n_stretch, 1, 2, po->d_ts_s, NULL, po->d_cost_s, NULL, hip_stream)) != 0) return r;
    }
    if (c.n_two && (r = solo_timescale(b, po->d_pcm_two, c.n_two, 2, 1, po->d_ts_a, NULL, po->d_cost_a, NULL, hip_stream)) != 0) return r;
    return solo_playout_render(po, d_streams, n, params, H, po->d_action, c.n_one, c.n_two, c.n_stretch, po->d_pcm_one, po->d_st_one, po->d_pcm_two, po->d_st_two,
                               po->d_ts_s, po->d_cost_s, po->d_ts_a, po->d_cost_a, d_heard, d_outcome, d_status, &d_count->render, hip_stream);
}

// ---- RTP at both ends (solo_rtp.h): records + pool -> datagrams for the socket; received datagrams -> arrivals, in place -------------
// A session is a row object whose record is a stream's configuration (a zeroed record = not bound: unbind is the listed reset), plus
// the sorted SSRC table and the host mirror both are rebuilt from.  The device code reads the configuration and never writes it.
static_assert(SX_RTP_CFG_WORDS <= SX_ROWS_MAX_WORDS, "solo_rtp.h and solo_rows.h agree");
struct solo_rtp_obj : solo_rows {    // d_state: SxRtpStream [n_rows]
    int32_t L;                       // timestamp ticks per packet
    SxRtpMirror mirror;
    uint32_t* d_table;               // SX_RTP_TABLE_HEAD + 2 x n_rows words
    void* d_scratch;                 // tile bases and tile totals of a solo_rtp_pack call, grown on demand
    size_t scratch_bytes;
    int32_t trailer;                 // solo_rtp_set_trailer
    // SRTP (solo_srtp.h): allocated by the first solo_srtp_set_keys.  The mirror holds tag lengths, never keys
    SxSrtpKey* d_keys;               // [n_rows][2]: tx, rx
    SxSrtpRx* d_rx;                  // [n_rows]
    SxSrtpMirror srtp;
    // SRTCP (solo_srtcp.h): ONE allocation (SxSrtcpMem) made by the first solo_srtcp_set_keys.  The mirror holds "has tx / has rx"
    void* d_srtcp;
    SxSrtcpMirror srtcp;
    // streams that hold a GCM key (solo_srtp_gcm.h): SRTP tx, SRTP rx, SRTCP tx, SRTCP rx -- counted wherever a mirror changes, so that a
    // device call asks "is the GCM kernel needed" without walking the mirror
    int32_t n_gcm[4];
};
static void rtp_count_gcm(solo_rtp_obj* r) {
    r->n_gcm[0] = sx_srtp_gcm_count(r->srtp.tx_tag); r->n_gcm[1] = sx_srtp_gcm_count(r->srtp.rx_tag);
    r->n_gcm[2] = sx_srtcp_gcm_count(r->srtcp.has_tx); r->n_gcm[3] = sx_srtcp_gcm_count(r->srtcp.has_rx);
}
solo_rtp_t* solo_rtp_create(int32_t n_streams, int32_t packet_samples) {
    if (n_streams <= 0 || (packet_samples != 320 && packet_samples != 640 && packet_samples != 1280) || !have_device()) return NULL;
    solo_rtp_obj* r = new (std::nothrow) solo_rtp_obj();
    if (!r) return NULL;
    r->L = packet_samples;
    r->mirror.cfg.assign((size_t)n_streams, SxRtpStream{0, 0, 0, 0});
    r->mirror.level_id = 0;
    const size_t table_bytes = (SX_RTP_TABLE_HEAD + 2 * (size_t)n_streams) * sizeof(uint32_t);
    if (hipMalloc((void**)&r->d_table, table_bytes) != hipSuccess || hipMemset(r->d_table, 0, table_bytes) != hipSuccess ||
        !rows_alloc(r, n_streams, SX_RTP_CFG_WORDS, NULL, 1, 0)) {
        solo_rtp_destroy(r);
        return NULL;
    }
    return r;
}
void solo_rtp_destroy(solo_rtp_t* r) {
    if (!r) return;
    if (r->d_keys) {                 // no key outlives the session in freed memory
        (void)hipMemset(r->d_keys, 0, 2 * (size_t)r->n_rows * sizeof(SxSrtpKey));
        (void)hipDeviceSynchronize();
    }
    if (r->d_srtcp) {
        (void)hipMemset(r->d_srtcp, 0, sx_srtcp_bytes(r->n_rows));
        (void)hipDeviceSynchronize();
    }
    dev_free(r->d_keys);
    dev_free(r->d_rx);
    dev_free(r->d_srtcp);
    rows_free(r);
    dev_free(r->d_table);
    dev_free(r->d_scratch);
    delete r;
}
// the new table, behind the kernels that changed the records; the call returns when it is there (the vector it came from goes)
static int32_t rtp_upload_table(solo_rtp_obj* r, const std::vector<u32>& table, hipStream_t st) {
    SOLO_CHECK(hipMemcpyAsync(r->d_table, table.data(), table.size() * sizeof(u32), hipMemcpyHostToDevice, st));
    SOLO_CHECK(hipStreamSynchronize(st));
    return 0;
}
int32_t solo_rtp_bind(solo_rtp_t* r, const int32_t* h_streams, int32_t n, const uint32_t* h_ssrc, const uint32_t* h_ts_offset, const uint16_t* h_seq_offset,
                      const uint8_t* h_pt_md1, const uint8_t* h_pt_md2, int32_t level_id, void* hip_stream) {
    std::vector<SxStreamCtl> recs;
    std::vector<u32> table;
    SxRtpMirror next;
    if (!r || !sx_rtp_bind_plan(r->mirror, h_streams, n, h_ssrc, h_ts_offset, h_seq_offset, h_pt_md1, h_pt_md2, level_id, next, recs, table)) return -1;
    hipStream_t st = (hipStream_t)hip_stream;
    SOLO_CHECK(sx_launch_ctl_batches(recs.data(), n, [&](const SxStreamCtlList& l, int k) {
        hipLaunchKernelGGL(solo_rtp_bind_kernel, dim3((unsigned)k), dim3(64), 0, st, (u32*)r->d_state, l);
    }));
    const int32_t e = rtp_upload_table(r, table, st);
    if (e == 0) r->mirror.cfg.swap(next.cfg), r->mirror.level_id = next.level_id;      // (only what the device now holds)
    return e;
}
// keys and receive records of the listed (validated) streams -> none; enqueued, the caller synchronises
static int32_t srtp_clear(solo_rtp_obj* r, const int32_t* h_streams, int32_t n, hipStream_t st) {
    if (!r->d_keys) return 0;
    for (int32_t i = 0; i < n; i++) {
        SOLO_CHECK(hipMemsetAsync(r->d_keys + 2 * (size_t)h_streams[i], 0, 2 * sizeof(SxSrtpKey), st));
        SOLO_CHECK(hipMemsetAsync(r->d_rx + h_streams[i], 0xFF, sizeof(i64), st));                                  // index = -1
        SOLO_CHECK(hipMemsetAsync((uint8_t*)(r->d_rx + h_streams[i]) + sizeof(i64), 0, sizeof(SxSrtpRx) - sizeof(i64), st));
        r->srtp.tx_tag[(size_t)h_streams[i]] = 0; r->srtp.rx_tag[(size_t)h_streams[i]] = 0;
    }
    rtp_count_gcm(r);
    return 0;
}
// SRTCP likewise: both keys and the send index to zero, the receive record to "none yet"
static int32_t srtcp_clear(solo_rtp_obj* r, const int32_t* h_streams, int32_t n, hipStream_t st) {
    if (!r->d_srtcp) return 0;
    const SxSrtcpMem m = sx_srtcp_mem(r->d_srtcp, r->n_rows);
    for (int32_t i = 0; i < n; i++) {
        SOLO_CHECK(hipMemsetAsync(m.keys + 2 * (size_t)h_streams[i], 0, 2 * sizeof(SxSrtpKey), st));
        SOLO_CHECK(hipMemsetAsync(m.tx + h_streams[i], 0, sizeof(SxSrtcpTx), st));
        SOLO_CHECK(hipMemsetAsync(&m.rx[h_streams[i]].index, 0xFF, sizeof(i64), st));                                // index = -1
        SOLO_CHECK(hipMemsetAsync(&m.rx[h_streams[i]].pending, 0, sizeof(u64), st));
        r->srtcp.has_tx[(size_t)h_streams[i]] = 0; r->srtcp.has_rx[(size_t)h_streams[i]] = 0;
    }
    rtp_count_gcm(r);
    return 0;
}
int32_t solo_rtp_unbind(solo_rtp_t* r, const int32_t* h_streams, int32_t n, void* hip_stream) {
    std::vector<u32> table;
    SxRtpMirror next;
    if (!r || !sx_rtp_unbind_plan(r->mirror, h_streams, n, next, table)) return -1;
    int32_t e = rows_reset_list(r, h_streams, n, (hipStream_t)hip_stream);
    if (e == 0) e = srtp_clear(r, h_streams, n, (hipStream_t)hip_stream);             // (a slot taken by the next bind inherits no key)
    if (e == 0) e = srtcp_clear(r, h_streams, n, (hipStream_t)hip_stream);
    if (e == 0) e = rtp_upload_table(r, table, (hipStream_t)hip_stream);
    if (e == 0) r->mirror.cfg.swap(next.cfg);
    return e;
}
int32_t solo_rtp_pack(solo_rtp_t* r, const solo_arrival_t* d_records, const solo_send_count_t* d_send_count, int32_t max_records, const uint8_t* d_payload,
                      int64_t payload_bytes, const uint8_t* d_level, int32_t level_depth, solo_dgram_t* d_dgrams, uint8_t* d_wire, int64_t wire_capacity,
                      solo_rtp_pack_count_t* d_count, void* hip_stream) {
    if (!r || !d_records || !d_send_count || !d_payload || !d_dgrams || !d_wire || !d_count || max_records <= 0 || payload_bytes < 0 || wire_capacity < 0) return -1;
    if (d_level && (level_depth <= 0 || r->mirror.level_id == 0)) return -1;       // (levels need the id the latest bind gave)
    if ((((uintptr_t)d_records | (uintptr_t)d_send_count | (uintptr_t)d_dgrams | (uintptr_t)d_wire) & 3) || ((uintptr_t)d_count & 7)) return -1;
    hipStream_t st = (hipStream_t)hip_stream;
    SOLO_CHECK(grow_scratch(r->d_scratch, r->scratch_bytes, solo_rtp_scratch_bytes(max_records), st));
    SxRtpPackArgs a;
    a.records = d_records; a.send_count = d_send_count; a.payload = d_payload; a.level = d_level;
    a.cfg = (const SxRtpStream*)r->d_state; a.table = r->d_table; a.payload_bytes = payload_bytes;
    a.max_records = max_records; a.n_streams = r->n_rows; a.level_depth = level_depth; a.packet_samples = r->L; a.trailer = r->trailer;
    SOLO_CHECK(solo_rtp_pack_launch(a, r->d_scratch, d_dgrams, d_wire, (long long)wire_capacity, d_count, st));
    return 0;
}
int32_t solo_rtp_parse(solo_rtp_t* r, solo_batch_t* b, const solo_dgram_t* d_dgrams, int32_t n_dgrams, const uint8_t* d_wire, int64_t wire_bytes,
                       solo_arrival_t* d_arrivals, uint8_t* d_level_out, uint16_t* d_rtp_seq_out, solo_rtp_parse_count_t* d_count, void* hip_stream) {
    if (!r || !b || !b->d_recv_ring || b->n_streams != r->n_rows || handle_packet_samples(b) != r->L) return -1;
    if (n_dgrams < 0 || wire_bytes < 0 || !d_count || (n_dgrams > 0 && (!d_dgrams || !d_wire || !d_arrivals))) return -1;
    if ((((uintptr_t)d_dgrams | (uintptr_t)d_arrivals | (uintptr_t)d_count) & 3) || ((uintptr_t)d_rtp_seq_out & 1)) return -1;
    SxRtpParseArgs a;
    a.dgrams = d_dgrams; a.wire = d_wire; a.cfg = (const SxRtpStream*)r->d_state; a.table = r->d_table; a.play = b->d_recv_play;
    a.wire_bytes = wire_bytes > 0x7FFFFFFFLL ? 0x7FFFFFFFLL : wire_bytes;
    a.n_dgrams = n_dgrams; a.n_streams = r->n_rows; a.packet_samples = r->L;
    SOLO_CHECK(solo_rtp_parse_launch(a, d_arrivals, d_level_out, d_rtp_seq_out, d_count, (hipStream_t)hip_stream));
    return 0;
}

// ---- SRTP (solo_srtp.h): the session's keys, then protect behind pack and unprotect in front of parse -----------------------------------
int32_t solo_rtp_set_trailer(solo_rtp_t* r, int32_t trailer_bytes) {
    if (!r || !sx_srtp_trailer_ok(r->srtp, trailer_bytes)) return -1;
    r->trailer = trailer_bytes;
    return 0;
}
// the planned records of a set_keys call of either transform (has_tx / has_rx: the directions it sets) -> the device, then the mirror
static int32_t srtp_put_keys(solo_rtp_obj* r, const int32_t* h_streams, int32_t n, bool has_tx, bool has_rx, std::vector<SxSrtpKey>& recs, const std::vector<SxSrtpRx>& rx,
                             SxSrtpMirror& next, hipStream_t st) {
    if (!r->d_keys) {                // the first call: every record "no key", every receive record "none yet"
        const size_t kb = 2 * (size_t)r->n_rows * sizeof(SxSrtpKey);
        std::vector<SxSrtpRx> none((size_t)r->n_rows);
        for (SxSrtpRx& x : none) { x.index = -1; x.pending = 0; x.roc0 = 0; x.pad[0] = x.pad[1] = x.pad[2] = 0; }
        if (hipMalloc((void**)&r->d_keys, kb) != hipSuccess || hipMalloc((void**)&r->d_rx, none.size() * sizeof(SxSrtpRx)) != hipSuccess ||
            hipMemset(r->d_keys, 0, kb) != hipSuccess || hipMemcpy(r->d_rx, none.data(), none.size() * sizeof(SxSrtpRx), hipMemcpyHostToDevice) != hipSuccess) {
            dev_free(r->d_keys);
            dev_free(r->d_rx);
            sx_srtp_wipe(recs);
            return -2;
        }
        r->srtp.tx_tag.assign((size_t)r->n_rows, 0); r->srtp.rx_tag.assign((size_t)r->n_rows, 0);
    }
    hipError_t e = hipSuccess;
    for (int32_t i = 0; i < n && e == hipSuccess; i++) {
        SxSrtpKey* d = r->d_keys + 2 * (size_t)h_streams[i];
        if (has_tx) e = hipMemcpyAsync(d, &recs[2 * (size_t)i], sizeof(SxSrtpKey), hipMemcpyHostToDevice, st);
        if (has_rx && e == hipSuccess) e = hipMemcpyAsync(d + 1, &recs[2 * (size_t)i + 1], sizeof(SxSrtpKey), hipMemcpyHostToDevice, st);
        if (has_rx && e == hipSuccess) e = hipMemcpyAsync(r->d_rx + h_streams[i], &rx[(size_t)i], sizeof(SxSrtpRx), hipMemcpyHostToDevice, st);
    }
    const hipError_t e2 = hipStreamSynchronize(st);         // (the host records go with this call: the copies must have read them)
    sx_srtp_wipe(recs);
    if (e != hipSuccess || e2 != hipSuccess) return -(int32_t)(e != hipSuccess ? e : e2);
    r->srtp.tx_tag.swap(next.tx_tag); r->srtp.rx_tag.swap(next.rx_tag);
    rtp_count_gcm(r);
    return 0;
}
int32_t solo_srtp_set_keys(solo_rtp_t* r, const int32_t* h_streams, int32_t n, const uint8_t* h_tx_master, const uint8_t* h_rx_master, const uint32_t* h_rx_roc,
                           int32_t tag_bytes, void* hip_stream) {
    std::vector<SxSrtpKey> recs;
    std::vector<SxSrtpRx> rx;
    SxSrtpMirror next;
    if (!r || !sx_srtp_set_keys_plan(r->srtp, r->n_rows, r->trailer, h_streams, n, h_tx_master, h_rx_master, h_rx_roc, tag_bytes, next, recs, rx)) return -1;
    return srtp_put_keys(r, h_streams, n, h_tx_master != NULL, h_rx_master != NULL, recs, rx, next, (hipStream_t)hip_stream);
}
int32_t solo_srtp_set_keys_gcm(solo_rtp_t* r, const int32_t* h_streams, int32_t n, const uint8_t* h_tx_master, const uint8_t* h_rx_master, const uint32_t* h_rx_roc,
                               void* hip_stream) {
    std::vector<SxSrtpKey> recs;
    std::vector<SxSrtpRx> rx;
    SxSrtpMirror next;
    if (!r || !sx_srtp_gcm_set_keys_plan(r->srtp, r->n_rows, r->trailer, h_streams, n, h_tx_master, h_rx_master, h_rx_roc, next, recs, rx)) return -1;
    return srtp_put_keys(r, h_streams, n, h_tx_master != NULL, h_rx_master != NULL, recs, rx, next, (hipStream_t)hip_stream);
}
int32_t solo_srtp_clear_keys(solo_rtp_t* r, const int32_t* h_streams, int32_t n, void* hip_stream) {
    if (!r || !sx_list_ok(h_streams, n, r->n_rows)) return -1;
    const int32_t e = srtp_clear(r, h_streams, n, (hipStream_t)hip_stream);
    SOLO_CHECK(hipStreamSynchronize((hipStream_t)hip_stream));
    return e;
}
int32_t solo_srtp_get_rx_index(solo_rtp_t* r, const int32_t* h_streams, int32_t n, int64_t* h_index, void* hip_stream) {
    if (!r || !h_index || !sx_list_ok(h_streams, n, r->n_rows)) return -1;
    for (int32_t i = 0; i < n; i++) h_index[i] = -1;
    if (!r->d_rx) return 0;
    hipStream_t st = (hipStream_t)hip_stream;
    for (int32_t i = 0; i < n; i++) SOLO_CHECK(hipMemcpyAsync(&h_index[i], &r->d_rx[h_streams[i]].index, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    SOLO_CHECK(hipStreamSynchronize(st));
    return 0;
}
int32_t solo_srtp_protect(solo_rtp_t* r, const solo_arrival_t* d_records, const solo_send_count_t* d_send_count, int32_t max_records, solo_dgram_t* d_dgrams,
                          uint8_t* d_wire, int64_t wire_bytes, solo_srtp_count_t* d_count, void* hip_stream) {
    if (!r || !d_records || !d_send_count || !d_dgrams || !d_wire || !d_count || max_records <= 0 || wire_bytes < 0) return -1;
    if (((uintptr_t)d_records | (uintptr_t)d_send_count | (uintptr_t)d_dgrams | (uintptr_t)d_count) & 3) return -1;
    SxSrtpProtectArgs a;
    a.records = d_records; a.send_count = d_send_count; a.dgrams = d_dgrams; a.wire = d_wire; a.cfg = (const SxRtpStream*)r->d_state; a.keys = r->d_keys;
    a.wire_bytes = wire_bytes > 0x7FFFFFFFLL ? 0x7FFFFFFFLL : wire_bytes;
    a.max_records = max_records; a.n_streams = r->n_rows;
    SOLO_CHECK(solo_srtp_protect_launch_all(a, d_count, r->n_gcm[0] > 0, (hipStream_t)hip_stream));
    return 0;
}
int32_t solo_srtp_unprotect(solo_rtp_t* r, const solo_dgram_t* d_dgrams, int32_t n_dgrams, uint8_t* d_wire, int64_t wire_bytes, solo_dgram_t* d_dgrams_out,
                            solo_srtp_count_t* d_count, void* hip_stream) {
    if (!r || n_dgrams < 0 || wire_bytes < 0 || !d_count || (n_dgrams > 0 && (!d_dgrams || !d_wire || !d_dgrams_out))) return -1;
    if (((uintptr_t)d_dgrams | (uintptr_t)d_dgrams_out | (uintptr_t)d_count) & 3) return -1;
    SxSrtpUnprotectArgs a;
    a.dgrams = d_dgrams; a.out = d_dgrams_out; a.wire = d_wire; a.table = r->d_table; a.keys = r->d_keys; a.rx = r->d_rx;
    a.wire_bytes = wire_bytes > 0x7FFFFFFFLL ? 0x7FFFFFFFLL : wire_bytes;
    a.n_dgrams = n_dgrams; a.n_streams = r->n_rows;
    SOLO_CHECK(solo_srtp_unprotect_launch_all(a, d_count, r->n_gcm[1] > 0, (hipStream_t)hip_stream));
    return 0;
}

// ---- forwarding without transcoding (solo_forward.h): a row object whose "row" is a room, K slots of four words each ----------------------
static_assert(SX_FWD_MAX_SLOTS * SX_FWD_SLOT_WORDS <= SX_ROWS_MAX_WORDS, "solo_forward.h and solo_rows.h agree");
struct solo_forward_obj : solo_rows {    // d_state: SxFwdSlot [n_rows][slots]; d_verdict[1]: the verdict word of the room plan
    int32_t slots;
    void* d_plan;                    // the room plan and the ranks (solo_forward_plan_bytes): sized at create
    void* d_scratch;                 // what a route call keeps per arrival (solo_forward_scratch_bytes), grown on demand
    size_t scratch_bytes;
};
solo_forward_t* solo_forward_create(int32_t n_rows, int32_t slots) {
    if (n_rows <= 0 || slots < 1 || slots > SX_FWD_MAX_SLOTS || (int64_t)n_rows * SX_FWD_MAX_SLOTS >= ((int64_t)1 << 31) || !have_device()) return NULL;
    solo_forward_obj* f = new (std::nothrow) solo_forward_obj();
    if (!f) return NULL;
    f->slots = slots;
    if (hipMalloc(&f->d_plan, solo_forward_plan_bytes(n_rows)) != hipSuccess || !rows_alloc(f, n_rows, slots * SX_FWD_SLOT_WORDS, sx_fwd_init_word, 1, 0)) {
        solo_forward_destroy(f);
        return NULL;
    }
    return f;
}
void solo_forward_destroy(solo_forward_t* f) {
    if (!f) return;
    rows_free(f);
    dev_free(f->d_plan);
    dev_free(f->d_scratch);
    delete f;
}
int32_t solo_forward_reset(solo_forward_t* f, void* hip_stream) { return rows_reset(f, (hipStream_t)hip_stream); }
int32_t solo_forward_reset_rooms(solo_forward_t* f, const int32_t* h_rooms, int32_t n, void* hip_stream) {
    return rows_reset_list(f, h_rooms, n, (hipStream_t)hip_stream);
}
int32_t solo_forward_get_state(solo_forward_t* f, const int32_t* d_rooms, int32_t n, uint8_t* d_blob, void* hip_stream) {
    return rows_copy_state(f, d_rooms, n, d_blob, 0, (hipStream_t)hip_stream);
}
int32_t solo_forward_set_state(solo_forward_t* f, const int32_t* d_rooms, int32_t n, const uint8_t* d_blob, void* hip_stream) {
    return rows_copy_state(f, d_rooms, n, (uint8_t*)d_blob, 1, (hipStream_t)hip_stream);
}
int32_t solo_forward_levels(const solo_arrival_t* d_arrivals, const uint8_t* d_level_in, int32_t n_dgrams, int32_t n_rows, int32_t default_level,
                            solo_forward_row_t* d_rowinfo, uint8_t* d_sa_q8, uint8_t* d_level, void* hip_stream) {
    if (!sx_fwd_levels_ok(d_arrivals, n_dgrams, n_rows, default_level, d_rowinfo, d_sa_q8, d_level)) return -1;
    SxFwdLevelArgs a;
    a.arrivals = d_arrivals; a.level_in = d_level_in; a.rowinfo = d_rowinfo; a.sa = d_sa_q8; a.level = d_level;
    a.n_dgrams = n_dgrams; a.n_rows = n_rows; a.default_level = default_level;
    SOLO_CHECK(solo_forward_levels_launch(a, (hipStream_t)hip_stream));
    return 0;
}
int32_t solo_forward_route(solo_forward_t* f, const solo_arrival_t* d_arrivals, int32_t n_dgrams, const solo_forward_row_t* d_rowinfo, const uint8_t* d_sel,
                           const int32_t* d_room, int32_t n, int32_t n_rooms, solo_arrival_t* d_records, int32_t max_records, solo_send_count_t* d_send_count,
                           uint8_t* d_level_fwd, int32_t* d_slot_src, solo_forward_count_t* d_count, void* hip_stream) {
    if (!sx_fwd_route_ok(f, f ? f->n_rows : 0, d_arrivals, n_dgrams, d_rowinfo, d_sel, d_room, n, n_rooms, d_records, max_records, d_send_count, d_slot_src,
                         d_count))
        return -1;
    hipStream_t st = (hipStream_t)hip_stream;
    SOLO_CHECK(grow_scratch(f->d_scratch, f->scratch_bytes, solo_forward_scratch_bytes(n_dgrams) + 16, st));
    SxFwdArgs a = {};
    a.arrivals = d_arrivals; a.rowinfo = d_rowinfo; a.sel = d_sel; a.room = d_room; a.state = (SxFwdSlot*)f->d_state;
    a.records = d_records; a.send_count = d_send_count; a.level_fwd = d_level_fwd; a.slot_src = d_slot_src; a.count = d_count;
    a.n_dgrams = n_dgrams; a.n = n; a.n_rooms = n_rooms; a.K = f->slots; a.max_records = max_records;
    SOLO_CHECK(solo_forward_route_launch(a, f->d_plan, f->n_rows, f->d_scratch, f->d_verdict, st));
    return 0;
}

// ---- RTCP (solo_rtcp.h): a row object beside the RTP sessions; d_extra: the CNAMEs, 8 words a row ------------------------------------------
static_assert(SX_RTCP_WORDS <= SX_ROWS_MAX_WORDS, "solo_rtcp.h and solo_rows.h agree");
struct solo_rtcp_obj : solo_rows {   // d_state: SxRtcpRow [n_rows]; d_verdict[2]: the verdict words of received's plan and of build's list
    void* d_plan;                    // what depends on the rows (solo_rtcp_plan_words): sized at create
    void* d_scratch;                 // what received and parse keep per datagram (solo_rtcp_scratch_bytes), grown on demand
    size_t scratch_bytes;
    int32_t trailer;                 // solo_rtcp_set_trailer
};
solo_rtcp_t* solo_rtcp_create(int32_t n_streams) {
    if (n_streams <= 0 || !have_device()) return NULL;
    solo_rtcp_obj* c = new (std::nothrow) solo_rtcp_obj();
    if (!c) return NULL;
    if (hipMalloc(&c->d_plan, solo_rtcp_plan_words(n_streams) * sizeof(i32)) != hipSuccess || !rows_alloc(c, n_streams, SX_RTCP_WORDS, NULL, 2, SX_RTCP_CNAME_WORDS)) {
        solo_rtcp_destroy(c);
        return NULL;
    }
    return c;
}
void solo_rtcp_destroy(solo_rtcp_t* c) {
    if (!c) return;
    rows_free(c);
    dev_free(c->d_plan);
    dev_free(c->d_scratch);
    delete c;
}
int32_t solo_rtcp_reset(solo_rtcp_t* c, void* hip_stream) { return rows_reset(c, (hipStream_t)hip_stream); }
int32_t solo_rtcp_reset_rows(solo_rtcp_t* c, const int32_t* h_rows, int32_t n, void* hip_stream) { return rows_reset_list(c, h_rows, n, (hipStream_t)hip_stream); }
int32_t solo_rtcp_get_state(solo_rtcp_t* c, const int32_t* d_rows, int32_t n, uint8_t* d_blob, void* hip_stream) {
    return rows_copy_state(c, d_rows, n, d_blob, 0, (hipStream_t)hip_stream);
}
int32_t solo_rtcp_set_state(solo_rtcp_t* c, const int32_t* d_rows, int32_t n, const uint8_t* d_blob, void* hip_stream) {
    return rows_copy_state(c, d_rows, n, (uint8_t*)d_blob, 1, (hipStream_t)hip_stream);
}
int32_t solo_rtcp_set_cname(solo_rtcp_t* c, const int32_t* h_streams, int32_t n, const char* h_cname, void* hip_stream) {
    if (!c || !sx_rtcp_cname_ok(h_streams, n, h_cname, c->n_rows)) return -1;
    hipStream_t st = (hipStream_t)hip_stream;
    hipError_t e = hipSuccess;
    for (int32_t i = 0; i < n && e == hipSuccess; i++)
        e = hipMemcpyAsync(c->d_extra + (size_t)h_streams[i] * SX_RTCP_CNAME_WORDS, h_cname + (size_t)i * SOLO_RTCP_CNAME_BYTES, SOLO_RTCP_CNAME_BYTES,
                           hipMemcpyHostToDevice, st);
    const hipError_t e2 = hipStreamSynchronize(st);         // (the caller's array goes with this call: the copies must have read it)
    SOLO_CHECK(e);
    SOLO_CHECK(e2);
    return 0;
}
int32_t solo_rtcp_received(solo_rtcp_t* c, const solo_rtp_t* r, const solo_arrival_t* d_arrivals, const uint16_t* d_rtp_seq, int32_t n_dgrams,
                           const uint32_t* d_arrival_time, uint32_t now_rtp, solo_rtcp_received_count_t* d_count, void* hip_stream) {
    if (!r || !sx_rtcp_received_ok(c, c ? c->n_rows : 0, r->n_rows, d_arrivals, d_rtp_seq, n_dgrams, d_arrival_time, d_count)) return -1;
    hipStream_t st = (hipStream_t)hip_stream;
    SOLO_CHECK(grow_scratch(c->d_scratch, c->scratch_bytes, solo_rtcp_scratch_bytes(n_dgrams), st));
    const SxRtcpPlanMem pm = sx_rtcp_plan_mem(c->d_plan, c->n_rows);
    SxRtcpRecvArgs a;
    a.arrivals = d_arrivals; a.rtp_seq = d_rtp_seq; a.arrival_time = d_arrival_time; a.cfg = (const SxRtpStream*)r->d_state; a.state = (SxRtcpRow*)c->d_state;
    a.key = (i32*)c->d_scratch; a.members = a.key + n_dgrams;
    a.counts = pm.counts; a.starts = pm.starts; a.cursor = pm.cursor; a.big = pm.big; a.count = (i32*)d_count;
    a.now_rtp = now_rtp; a.n_dgrams = n_dgrams; a.n_streams = c->n_rows; a.packet_samples = r->L;
    SOLO_CHECK(solo_rtcp_received_launch(a, c->d_verdict, st));
    return 0;
}
int32_t solo_rtcp_sent(solo_rtcp_t* c, const solo_rtp_t* r, const solo_arrival_t* d_records, const solo_send_count_t* d_send_count, int32_t max_records,
                       const solo_dgram_t* d_dgrams, solo_rtcp_sent_count_t* d_count, void* hip_stream) {
    if (!r || !sx_rtcp_sent_ok(c, c ? c->n_rows : 0, r->n_rows, d_records, d_send_count, max_records, d_dgrams, d_count)) return -1;
    SxRtcpSentArgs a;
    a.records = d_records; a.send_count = d_send_count; a.dgrams = d_dgrams; a.state = (SxRtcpRow*)c->d_state; a.count = (i32*)d_count;
    a.max_records = max_records; a.n_streams = c->n_rows;
    SOLO_CHECK(solo_rtcp_sent_launch(a, (hipStream_t)hip_stream));
    return 0;
}
int32_t solo_rtcp_build(solo_rtcp_t* c, const solo_rtp_t* r_tx, const solo_rtp_t* r_rx, const int32_t* d_streams, int32_t n, uint64_t now_ntp,
                        const uint64_t* d_now_ntp, solo_dgram_t* d_dgrams, uint8_t* d_wire, int64_t wire_capacity, solo_rtcp_build_count_t* d_count,
                        void* hip_stream) {
    if (!r_tx || !sx_rtcp_build_ok(c, c ? c->n_rows : 0, r_tx->n_rows, r_rx != NULL, r_rx ? r_rx->n_rows : 0, d_streams, n, d_now_ntp, d_dgrams, d_wire,
                                   wire_capacity, d_count))
        return -1;
    hipStream_t st = (hipStream_t)hip_stream;
    const SxRtcpPlanMem pm = sx_rtcp_plan_mem(c->d_plan, c->n_rows);
    SxRtcpBuildArgs a;
    a.streams = d_streams; a.cfg_tx = (const SxRtpStream*)r_tx->d_state; a.cfg_rx = r_rx ? (const SxRtpStream*)r_rx->d_state : NULL;
    a.state = (SxRtcpRow*)c->d_state; a.cname = (const u32*)c->d_extra; a.d_now = (const unsigned long long*)d_now_ntp; a.now = now_ntp;
    a.dgrams = d_dgrams; a.wire = d_wire; a.cap = wire_capacity; a.count = d_count; a.totals = pm.totals; a.bases = pm.bases;
    a.n = n; a.n_streams = c->n_rows; a.packet_samples = r_tx->L; a.trailer = c->trailer;
    SOLO_CHECK(launch_list_check(d_streams, n, c->n_rows, c->d_verdict + 1, NULL, st));
    SOLO_CHECK(solo_rtcp_build_launch(a, c->d_verdict + 1, st));
    return 0;
}
int32_t solo_rtcp_parse(solo_rtcp_t* c, const solo_rtp_t* r_rx, const solo_rtp_t* r_tx, const solo_dgram_t* d_dgrams, int32_t n_dgrams, const uint8_t* d_wire,
                        int64_t wire_bytes, uint64_t now_ntp, const uint64_t* d_now_ntp, solo_rtcp_feedback_t* d_feedback, solo_rtcp_parse_count_t* d_count,
                        void* hip_stream) {
    if (!r_rx || !sx_rtcp_parse_ok(c, c ? c->n_rows : 0, r_rx->n_rows, r_tx != NULL, r_tx ? r_tx->n_rows : 0, d_dgrams, n_dgrams, d_wire, wire_bytes, d_now_ntp,
                                   d_feedback, d_count))
        return -1;
    hipStream_t st = (hipStream_t)hip_stream;
    SOLO_CHECK(grow_scratch(c->d_scratch, c->scratch_bytes, solo_rtcp_scratch_bytes(n_dgrams), st));
    const SxRtcpPlanMem pm = sx_rtcp_plan_mem(c->d_plan, c->n_rows);
    SxRtcpParseArgs a;
    a.dgrams = d_dgrams; a.wire = d_wire; a.table_rx = r_rx->d_table; a.table_tx = r_tx ? r_tx->d_table : NULL; a.state = (SxRtcpRow*)c->d_state;
    a.win = pm.win; a.ok = (i32*)c->d_scratch; a.feedback = d_feedback; a.count = (i32*)d_count;
    a.d_now = (const unsigned long long*)d_now_ntp; a.now = now_ntp;
    a.wire_bytes = wire_bytes > 0x7FFFFFFFLL ? 0x7FFFFFFFLL : wire_bytes;
    a.n_dgrams = n_dgrams; a.n_streams = c->n_rows;
    SOLO_CHECK(solo_rtcp_parse_launch(a, st));
    return 0;
}

// ---- SRTCP (solo_srtcp.h): the session's RTCP keys and indices, protect behind solo_rtcp_build, unprotect in front of solo_rtcp_parse -------
int32_t solo_rtcp_set_trailer(solo_rtcp_t* c, int32_t trailer_bytes) {
    if (!c || !sx_srtcp_trailer_ok(trailer_bytes)) return -1;
    c->trailer = trailer_bytes;
    return 0;
}
// the planned records of a set_keys call of either transform -> the device, then the mirror
static int32_t srtcp_put_keys(solo_rtp_obj* r, const int32_t* h_streams, int32_t n, bool has_tx, bool has_rx, std::vector<SxSrtpKey>& recs, const std::vector<SxSrtcpTx>& tx,
                              const std::vector<SxSrtcpRx>& rx, SxSrtcpMirror& next, hipStream_t st) {
    if (!r->d_srtcp) {               // the first call: every record "no key", every send index 0, every receive record "none yet"
        const size_t bytes = sx_srtcp_bytes(r->n_rows);
        std::vector<u8> init(bytes);
        sx_srtcp_mem_init(init.data(), r->n_rows);
        if (hipMalloc(&r->d_srtcp, bytes) != hipSuccess || hipMemcpy(r->d_srtcp, init.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) {
            dev_free(r->d_srtcp);
            sx_srtp_wipe(recs);
            return -2;
        }
        r->srtcp.has_tx.assign((size_t)r->n_rows, 0); r->srtcp.has_rx.assign((size_t)r->n_rows, 0);
    }
    const SxSrtcpMem m = sx_srtcp_mem(r->d_srtcp, r->n_rows);
    hipError_t e = hipSuccess;
    for (int32_t i = 0; i < n && e == hipSuccess; i++) {
        const size_t s = (size_t)h_streams[i];
        if (has_tx) e = hipMemcpyAsync(m.keys + 2 * s, &recs[2 * (size_t)i], sizeof(SxSrtpKey), hipMemcpyHostToDevice, st);
        if (has_tx && e == hipSuccess) e = hipMemcpyAsync(m.tx + s, &tx[(size_t)i], sizeof(SxSrtcpTx), hipMemcpyHostToDevice, st);
        if (has_rx && e == hipSuccess) e = hipMemcpyAsync(m.keys + 2 * s + 1, &recs[2 * (size_t)i + 1], sizeof(SxSrtpKey), hipMemcpyHostToDevice, st);
        if (has_rx && e == hipSuccess) e = hipMemcpyAsync(m.rx + s, &rx[(size_t)i], sizeof(SxSrtcpRx), hipMemcpyHostToDevice, st);
    }
    const hipError_t e2 = hipStreamSynchronize(st);         // (the host records go with this call: the copies must have read them)
    sx_srtp_wipe(recs);
    if (e != hipSuccess || e2 != hipSuccess) return -(int32_t)(e != hipSuccess ? e : e2);
    r->srtcp.has_tx.swap(next.has_tx); r->srtcp.has_rx.swap(next.has_rx);
    rtp_count_gcm(r);
    return 0;
}
int32_t solo_srtcp_set_keys(solo_rtp_t* r, const int32_t* h_streams, int32_t n, const uint8_t* h_tx_master, const uint8_t* h_rx_master, const uint32_t* h_tx_index,
                            const int64_t* h_rx_index, void* hip_stream) {
    std::vector<SxSrtpKey> recs;
    std::vector<SxSrtcpTx> tx;
    std::vector<SxSrtcpRx> rx;
    SxSrtcpMirror next;
    if (!r || !sx_srtcp_set_keys_plan(r->srtcp, r->n_rows, h_streams, n, h_tx_master, h_rx_master, h_tx_index, (const i64*)h_rx_index, next, recs, tx, rx)) return -1;
    return srtcp_put_keys(r, h_streams, n, h_tx_master != NULL, h_rx_master != NULL, recs, tx, rx, next, (hipStream_t)hip_stream);
}
int32_t solo_srtcp_set_keys_gcm(solo_rtp_t* r, const int32_t* h_streams, int32_t n, const uint8_t* h_tx_master, const uint8_t* h_rx_master, const uint32_t* h_tx_index,
                                const int64_t* h_rx_index, void* hip_stream) {
    std::vector<SxSrtpKey> recs;
    std::vector<SxSrtcpTx> tx;
    std::vector<SxSrtcpRx> rx;
    SxSrtcpMirror next;
    if (!r || !sx_srtcp_gcm_set_keys_plan(r->srtcp, r->n_rows, h_streams, n, h_tx_master, h_rx_master, h_tx_index, (const i64*)h_rx_index, next, recs, tx, rx)) return -1;
    return srtcp_put_keys(r, h_streams, n, h_tx_master != NULL, h_rx_master != NULL, recs, tx, rx, next, (hipStream_t)hip_stream);
}
int32_t solo_srtcp_clear_keys(solo_rtp_t* r, const int32_t* h_streams, int32_t n, void* hip_stream) {
    if (!r || !sx_list_ok(h_streams, n, r->n_rows)) return -1;
    const int32_t e = srtcp_clear(r, h_streams, n, (hipStream_t)hip_stream);
    SOLO_CHECK(hipStreamSynchronize((hipStream_t)hip_stream));
    return e;
}
int32_t solo_srtcp_get_index(solo_rtp_t* r, const int32_t* h_streams, int32_t n, uint32_t* h_tx_next, int64_t* h_rx_index, void* hip_stream) {
    if (!r || !sx_list_ok(h_streams, n, r->n_rows)) return -1;
    for (int32_t i = 0; i < n; i++) {
        if (h_tx_next) h_tx_next[i] = 0;
        if (h_rx_index) h_rx_index[i] = -1;
    }
    if (!r->d_srtcp) return 0;
    const SxSrtcpMem m = sx_srtcp_mem(r->d_srtcp, r->n_rows);
    hipStream_t st = (hipStream_t)hip_stream;
    for (int32_t i = 0; i < n; i++) {
        if (h_tx_next) SOLO_CHECK(hipMemcpyAsync(&h_tx_next[i], &m.tx[h_streams[i]].next, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        if (h_rx_index) SOLO_CHECK(hipMemcpyAsync(&h_rx_index[i], &m.rx[h_streams[i]].index, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    }
    SOLO_CHECK(hipStreamSynchronize(st));
    return 0;
}
int32_t solo_srtcp_protect(const solo_rtcp_t* c, solo_rtp_t* r_tx, const int32_t* d_streams, int32_t n, const solo_rtcp_build_count_t* d_build_count,
                           solo_dgram_t* d_dgrams, uint8_t* d_wire, int64_t wire_bytes, solo_srtcp_count_t* d_count, void* hip_stream) {
    if (!sx_srtcp_protect_ok(c, c ? c->n_rows : 0, c ? c->trailer : 0, r_tx, r_tx ? r_tx->n_rows : 0, d_streams, n, d_build_count, d_dgrams, d_wire, wire_bytes,
                             d_count) ||
        !sx_srtcp_gcm_protect_ok(r_tx->n_gcm[2] > 0, c->trailer))
        return -1;
    const SxSrtcpMem m = sx_srtcp_mem(r_tx->d_srtcp, r_tx->n_rows);
    SxSrtcpProtectArgs a;
    a.streams = d_streams; a.build_count = d_build_count; a.dgrams = d_dgrams; a.wire = d_wire; a.keys = m.keys; a.tx = m.tx;
    a.wire_bytes = wire_bytes > 0x7FFFFFFFLL ? 0x7FFFFFFFLL : wire_bytes;
    a.n = n; a.n_streams = r_tx->n_rows;
    SOLO_CHECK(solo_srtcp_protect_launch_all(a, d_count, r_tx->n_gcm[2] > 0, (hipStream_t)hip_stream));
    return 0;
}
int32_t solo_srtcp_unprotect(solo_rtp_t* r_rx, const solo_dgram_t* d_dgrams, int32_t n_dgrams, uint8_t* d_wire, int64_t wire_bytes, solo_dgram_t* d_dgrams_out,
                             solo_srtcp_count_t* d_count, void* hip_stream) {
    if (!sx_srtcp_unprotect_ok(r_rx, d_dgrams, n_dgrams, d_wire, wire_bytes, d_dgrams_out, d_count)) return -1;
    const SxSrtcpMem m = sx_srtcp_mem(r_rx->d_srtcp, r_rx->n_rows);
    SxSrtcpUnprotectArgs a;
    a.dgrams = d_dgrams; a.out = d_dgrams_out; a.wire = d_wire; a.table = r_rx->d_table; a.keys = m.keys; a.rx = m.rx;
    a.wire_bytes = wire_bytes > 0x7FFFFFFFLL ? 0x7FFFFFFFLL : wire_bytes;
    a.n_dgrams = n_dgrams; a.n_streams = r_rx->n_rows;
    SOLO_CHECK(solo_srtcp_unprotect_launch_all(a, d_count, r_rx->n_gcm[3] > 0, (hipStream_t)hip_stream));
    return 0;
}

// ---- stream migration (solo_migrate.h): encoder state, decoder state and receive queue of listed streams <-> a device blob ---------
// which: a non-empty subset of {1 encoder, 2 decoder, 4 receive queue} that the handle has
static bool migrate_which_ok(const solo_batch* b, int32_t which) {
    return b && which > 0 && which <= SX_MIG_ALL && !((which & SX_MIG_ENC) && !b->have_enc) && !((which & SX_MIG_DEC) && !b->have_dec) &&
           !((which & SX_MIG_RECV) && !b->d_recv_ring);
}
static SxMigHandle migrate_handle(const solo_batch* b) {
    SxMigHandle h;
    memset(&h, 0, sizeof(h));
    h.n_streams = b->n_streams;
#ifdef SOLO_WITH_ENCODER
    if (b->have_enc) {
        h.enc = (uint8_t*)b->d_enc_state;
        h.g.enc_rate = b->enc_ctrl.samplerate; h.g.enc_mode = sx_mig_mode(enc_frames_per_packet(b), enc_hb_joint(b)); h.g.enc_bytes = (int32_t)b->eops->state_bytes;
    }
#endif
    if (b->have_dec) {
        h.dec = (uint8_t*)b->d_dec_state;
        h.g.dec_rate = b->dec_ctrl.samplerate;
        h.g.dec_mode = sx_mig_mode(ctrl_frames_per_packet(b->dec_ctrl.framesize_ms), ctrl_hb_joint(b->dec_ctrl.joint_enable, b->dec_ctrl.joint_mode));
        h.g.dec_bytes = (int32_t)b->dops->state_bytes;
    }
    if (b->d_recv_ring) {
        h.ring = b->d_recv_ring; h.lens = b->d_recv_lens; h.play = b->d_recv_play; h.trk = b->d_recv_trk;
        h.g.depth = b->recv_depth; h.g.slot = b->recv_slot;
    }
    return h;
}
int64_t solo_batch_state_bytes(const solo_batch_t* b, int32_t which) {
    if (!migrate_which_ok(b, which)) return -1;
    const SxMigHandle h = migrate_handle(b);
    return SX_MIG_HDR_BYTES + sx_mig_body_bytes(sx_mig_geom_of(h.g, which), which);
}
static bool migrate_args_ok(const solo_batch* b, const int32_t* d_streams, int32_t n, int32_t which, const uint8_t* d_blob, int64_t blob_stride,
                            const solo_migrate_count_t* d_count) {
    if (!migrate_which_ok(b, which) || !d_streams || !d_blob || !d_count || n <= 0 || n > b->n_streams) return false;
    return blob_stride >= solo_batch_state_bytes(b, which) && !(blob_stride & 15) && !((uintptr_t)d_blob & 15);
}
int32_t solo_batch_export_streams(solo_batch_t* b, const int32_t* d_streams, int32_t n, int32_t which, uint8_t* d_blob, int64_t blob_stride,
                                  solo_migrate_count_t* d_count, void* hip_stream) {
    if (!migrate_args_ok(b, d_streams, n, which, d_blob, blob_stride, d_count)) return -1;
    hipStream_t st = (hipStream_t)hip_stream;
    {   // (the states must be those the work in flight leaves behind)
        const int32_t r = solo_wait_in_flight(b, st);
        if (r) return r;
    }
    uint32_t* verdict = b->d_verdict + SOLO_VERDICT_EXPORT;
    SOLO_CHECK(launch_list_check(d_streams, n, b->n_streams, verdict, NULL, st));
    SOLO_CHECK(solo_migrate_export_launch(migrate_handle(b), d_streams, n, which, d_blob, (long long)blob_stride, d_count, verdict, st));
    return 0;
}
int32_t solo_batch_import_streams(solo_batch_t* b, const int32_t* d_streams, int32_t n, int32_t which, const uint8_t* d_blob, int64_t blob_stride,
                                  solo_migrate_count_t* d_count, void* hip_stream) {
    if (!migrate_args_ok(b, d_streams, n, which, d_blob, blob_stride, d_count)) return -1;
    hipStream_t st = (hipStream_t)hip_stream;
    {   // (as solo_batch_reset_streams: the kernels in flight write whole states back when they end)
        const int32_t r = solo_wait_in_flight(b, st);
        if (r) return r;
    }
    uint32_t* verdict = b->d_verdict + SOLO_VERDICT_IMPORT;
    SOLO_CHECK(launch_list_check(d_streams, n, b->n_streams, verdict, NULL, st));
    SOLO_CHECK(solo_migrate_import_launch(migrate_handle(b), d_streams, n, which, d_blob, (long long)blob_stride, d_count, verdict, st));
    return 0;
}

#ifdef SOLO_WITH_ENCODER
// map = NULL: every stream (solo_batch_encode); else the n listed streams of solo_batch_encode_streams: PCM, payloads, status and the
// hand-over records at the compact position, the stream state through the map (solo_stream_ctl.h).  The schedules: solo_enc_pipe.h
static int32_t solo_encode_impl(solo_batch_t* b, const int32_t* map, int32_t n, const int16_t* d_pcm, int32_t n_packets, uint8_t* d_bits, int16_t* d_nbytes,
                                int32_t* d_status, hipStream_t st) {
    const size_t np = (size_t)b->n_streams * (size_t)n_packets;
    const solo_enc_ops* ops = b->eops;
    solo_enc_pipe* p = &b->enc;
    // a subset call's quantiser addresses the states of its rows with 32-bit offsets from the handle's first state (solo_nsq_row.hip)
    if (map && (unsigned long long)b->n_streams * (unsigned long long)ops->state_bytes >= (1ull << 32)) return -1;
    // the quantiser addresses the hand-over records of its wavefront's four streams with 32-bit offsets from a wave-uniform base
    // (solo_nsq_row.hip): the records of 3 streams x 2 n_packets, plus one more record for the offsets inside the last one, must stay
    // below 4 GiB (~700 k packets per call at the 16 kHz API rate)
    const unsigned long long per_wave = 64ull / (unsigned long long)ops->nsq_workgroups(64);
    if (((per_wave - 1ull) * 2ull * (unsigned long long)n_packets + 1ull) * (unsigned long long)ops->nsq_out_bytes >= (1ull << 32)) return -1;
    int32_t r;
    if (!p->ready && (r = enc_pipe_setup(p, ops, b->n_streams, b->slot, enc_packet_samples(b))) != 0) return r;
    const size_t sz_in = np * 2 * ops->nsq_in_bytes, sz_out = np * 2 * ops->nsq_out_bytes, sz_code = np * ops->code_in_bytes;
    if (sz_in + sz_out + sz_code + 256 > p->enc_work_bytes) {          // the hand-over area grows (synchronises; steady-state calls do not)
        (void)hipStreamSynchronize(p->sA); (void)hipStreamSynchronize(p->sB); (void)hipStreamSynchronize(p->sC);
    }
    SOLO_CHECK(grow_scratch(p->d_enc_work, p->enc_work_bytes, sz_in + sz_out + sz_code + 256, st));
    enc_rows call = {0, map ? n : b->n_streams, b->d_enc_state, map, d_pcm, NULL, NULL, NULL, d_bits, d_nbytes, d_status};
    call.nin = p->d_enc_work;
    call.nout = (char*)call.nin + ((sz_in + 63) & ~(size_t)63);
    call.cin = (char*)call.nout + ((sz_out + 63) & ~(size_t)63);
    // SOLO_ENC_PERSIST=1: calls of two or more packets run the persistent schedule (a single packet has nothing to pipeline inside the call);
    // a subset call always runs the launch-per-chunk schedule
    if (!map && p->persist && n_packets >= 2) return enc_pipe_run_persist(p, call, n_packets, b->timing != 0, st);
    uint32_t* verdict = NULL;
    if (map) {
        // the verdict word of this call; the call two before used the same one: its kernels must be through
        const unsigned long long cap = stream_capture(st);
        verdict = b->d_verdict + SOLO_VERDICT_ENC + enc_pipe_call_set(p, -1, cap);
        SOLO_CHECK(enc_pipe_wait(p, st, cap, 1, ENC_END));
        SOLO_CHECK(launch_list_check(map, n, b->n_streams, verdict, d_status, st));
    }
    return enc_pipe_run_chunks(p, call, n_packets, verdict, b->timing != 0, st);
}
// Asynchronous joins: with on = 1 solo_batch_encode returns without making the caller's stream wait for its internal streams, so
// that the next encode call can start (its first analysis chunk) while the last quantiser / coding chunks of this one still run.
// Whoever consumes the outputs then calls solo_batch_wait_encode(b, stream, which) first: which = 0 the most recent encode call,
// 1 the one before.  The hand-over records are guarded inside the library; the OUTPUT buffers of two calls in flight must differ.
int32_t solo_batch_set_async_join(solo_batch_t* b, int32_t on) {
    if (!b) return -1;
    b->enc.async_join = on ? 1 : 0;
    return 0;
}
int32_t solo_batch_wait_encode(solo_batch_t* b, void* hip_stream, int32_t which) {
    if (!b || which < 0 || which > 1) return b ? 0 : -1;
    // (a call issued on the other side of a capture is not waited for: stream order, see stream_capture)
    SOLO_CHECK(enc_pipe_wait(&b->enc, (hipStream_t)hip_stream, stream_capture((hipStream_t)hip_stream), which, ENC_END));
    return 0;
}
int32_t solo_batch_last_encode_chunks(const solo_batch_t* b) { return b ? b->enc.last_chunks : 0; }
int32_t solo_batch_encode(solo_batch_t* b, const int16_t* d_pcm, int32_t n_packets, uint8_t* d_bits, int16_t* d_nbytes,
                          int32_t* d_status, void* hip_stream) {
    if (!b || !b->have_enc || !d_pcm || !d_bits || !d_nbytes || n_packets <= 0) return -1;
    return solo_encode_impl(b, NULL, 0, d_pcm, n_packets, d_bits, d_nbytes, d_status, (hipStream_t)hip_stream);
}
int32_t solo_batch_encode_streams(solo_batch_t* b, const int32_t* d_streams, int32_t n, const int16_t* d_pcm, int32_t n_packets, uint8_t* d_bits,
                                  int16_t* d_nbytes, int32_t* d_status, void* hip_stream) {
    if (!b || !b->have_enc || !d_streams || n <= 0 || n > b->n_streams || !d_pcm || !d_bits || !d_nbytes || n_packets <= 0) return -1;
    return solo_encode_impl(b, d_streams, n, d_pcm, n_packets, d_bits, d_nbytes, d_status, (hipStream_t)hip_stream);
}
#else
int32_t solo_batch_encode(solo_batch_t*, const int16_t*, int32_t, uint8_t*, int16_t*, int32_t*, void*) { return -1; }
int32_t solo_batch_encode_streams(solo_batch_t*, const int32_t*, int32_t, const int16_t*, int32_t, uint8_t*, int16_t*, int32_t*, void*) { return -1; }
int32_t solo_batch_set_async_join(solo_batch_t* b, int32_t) { return b ? 0 : -1; }
int32_t solo_batch_wait_encode(solo_batch_t* b, void*, int32_t) { return b ? 0 : -1; }
int32_t solo_batch_last_encode_chunks(const solo_batch_t*) { return 0; }
#endif

// ---- the reference's six entry points: a batch of one stream, staged through device buffers ----------
struct solo_single {
    solo_batch* b;
    // One device block and one pinned host block of the same layout: [status 16 B][pcm 2 x 1280 B][nbytes 16 B][bits: slot bytes].
    // A call is one host-to-device copy, the kernels, one device-to-host copy and ONE synchronisation (round 2 made three synchronous
    // copies per call: 0.26 ms per decoded packet against 0.024 ms of the reference on a host core, tools/legacy_api_cost.py).
    uint8_t* d_blk;
    uint8_t* h_blk;
    int16_t* d_pcm;
    uint8_t* d_bits;
    int16_t* d_nbytes;
    int32_t* d_status;
    int is_enc;
};
#define SOLO_SINGLE_PCM_OFF 16
#define SOLO_SINGLE_NB_OFF (16 + 2 * SX_PACKET * 2)
#define SOLO_SINGLE_BITS_OFF (SOLO_SINGLE_NB_OFF + 16)

static void single_free(solo_single* h) {
    if (!h) return;
    if (h->d_blk) (void)hipFree(h->d_blk);
    if (h->h_blk) (void)hipHostFree(h->h_blk);
    solo_batch_destroy(h->b);
    free(h);
}

static solo_single* single_new(const USER_Ctrl_enc* e, const USER_Ctrl_dec* d) {
    solo_single* h = (solo_single*)calloc(1, sizeof(solo_single));
    if (!h) return NULL;
    h->is_enc = e != NULL;
    h->b = solo_batch_create(1, e, d, 1024 + 64);   // MAX_FRAME_BYTES of the reference harness + slack
    const size_t blk = h->b ? (size_t)SOLO_SINGLE_BITS_OFF + (size_t)h->b->slot : 0;
    // A call moves ~1.4 KB each way through one pinned host block and one device block of the same layout.  (Letting the kernels address the
    // pinned block directly -- no staging copies -- measured the same 0.21 ms per decode call: the call is its single-wave kernel chain + one
    // synchronisation.)
    if (!h->b || hipHostMalloc((void**)&h->h_blk, blk, hipHostMallocDefault) != hipSuccess) { single_free(h); return NULL; }
    memset(h->h_blk, 0, blk);
    if (hipMalloc((void**)&h->d_blk, blk) != hipSuccess || hipMemset(h->d_blk, 0, blk) != hipSuccess) {
        single_free(h);
        return NULL;
    }
    h->d_status = (int32_t*)h->d_blk;
    h->d_pcm = (int16_t*)(h->d_blk + SOLO_SINGLE_PCM_OFF);
    h->d_nbytes = (int16_t*)(h->d_blk + SOLO_SINGLE_NB_OFF);
    h->d_bits = h->d_blk + SOLO_SINGLE_BITS_OFF;
    return h;
}

void* AGR_Sate_Encoder_Init(USER_Ctrl_enc* enc_Ctrl) {
    if (!enc_Ctrl) return NULL;
    if (enc_Ctrl->targetRate_bps <= 0) enc_Ctrl->targetRate_bps = 15600;   // the reference rewrites the caller's struct
    return single_new(enc_Ctrl, NULL);
}

int32_t AGR_Sate_Encoder_Encode(void* st, const int16_t* pcm, uint8_t* bits, int32_t bufSize, int16_t* nBytesOut) {
    solo_single* h = (solo_single*)st;
    if (!h || !h->is_enc) return -1;
    const size_t pcm_bytes = (size_t)enc_packet_samples(h->b) * 2;      // JC1_FrameSize samples
    memcpy(h->h_blk + SOLO_SINGLE_PCM_OFF, pcm, pcm_bytes);
    if (hipMemcpyAsync(h->d_pcm, h->h_blk + SOLO_SINGLE_PCM_OFF, pcm_bytes, hipMemcpyHostToDevice, (hipStream_t)0) != hipSuccess) return -1;
    if (solo_batch_encode(h->b, h->d_pcm, 1, h->d_bits, h->d_nbytes, h->d_status, NULL) != 0) return -1;
    // lengths + the whole payload slot in one copy (a payload is at most a few hundred bytes; the slot 1088)
    if (hipMemcpyAsync(h->h_blk + SOLO_SINGLE_NB_OFF, h->d_blk + SOLO_SINGLE_NB_OFF, 16 + (size_t)h->b->slot, hipMemcpyDeviceToHost, (hipStream_t)0) != hipSuccess) return -1;
    if (hipStreamSynchronize((hipStream_t)0) != hipSuccess) return -1;
    int16_t nb[2];
    memcpy(nb, h->h_blk + SOLO_SINGLE_NB_OFF, 4);
    int32_t n = nb[0];
    if (n == 0 && h->b->enc_ctrl.dtx_enable)                                 // DTX packet: the reference still returns the high-band bytes
        n = ctrl_hb_bytes(h->b->enc_ctrl.joint_enable, h->b->enc_ctrl.joint_mode, h->b->enc_ctrl.framesize_ms);
    if (n > bufSize) n = bufSize;                                            // AGR_Sate_bits_write truncates to max_nbytes
    if (n > h->b->slot) n = h->b->slot;
    if (n > 0) memcpy(bits, h->h_blk + SOLO_SINGLE_BITS_OFF, (size_t)n);
    nBytesOut[0] = nb[0];
    nBytesOut[1] = nb[1];
    return n;
}

int AGR_Sate_Encoder_Uninit(void* st) {
    if (!st) return -1;
    single_free((solo_single*)st);
    return 0;
}

void* AGR_Sate_Decoder_Init(USER_Ctrl_dec* dec_Ctrl) {
    if (!dec_Ctrl) return NULL;
    return single_new(NULL, dec_Ctrl);
}

int32_t AGR_Sate_Decoder_Decode(void* st, int16_t* pcm, int16_t* nSamplesOut, const uint8_t* bits, int16_t nBytes[], int32_t lostflag) {
    solo_single* h = (solo_single*)st;
    if (!h || h->is_enc) return -1;
    if (nBytes[0] <= 0) return -1;                                           // AGR_BWE_SDK_API.c:266 (state untouched, outputs unwritten)
    if (lostflag < 1 || lostflag > 4) return -1;
    const int ns = dec_packet_samples(h->b);                                 // JC1_FrameSize (AGR_BWE_SDK_API.c:277)
    const int32_t hbb = ctrl_hb_bytes(h->b->dec_ctrl.joint_enable, h->b->dec_ctrl.joint_mode, h->b->dec_ctrl.framesize_ms);
    int32_t n0 = nBytes[0], n1 = nBytes[1];
    if (lostflag != 1) {
        // lengths that do not describe bytes inside the caller's buffer are refused before anything is read (the reference would
        // read out of bounds): too long -> SKP_SILK_DEC_PAYLOAD_TOO_LARGE, inconsistent -> SKP_SILK_DEC_PAYLOAD_ERROR
        if (n0 > h->b->slot) { *nSamplesOut = (int16_t)ns; return -11; }
        if (n1 < 0 || n1 > n0 || (n1 > 0 && n1 < hbb) || (lostflag == 3 && n0 <= hbb) || (lostflag == 4 && n0 < hbb)) { *nSamplesOut = (int16_t)ns; return -12; }
        memcpy(h->h_blk + SOLO_SINGLE_BITS_OFF, bits, (size_t)n0);
        if (hipMemcpyAsync(h->d_bits, h->h_blk + SOLO_SINGLE_BITS_OFF, (size_t)n0, hipMemcpyHostToDevice, (hipStream_t)0) != hipSuccess) return -1;
    }
    if (h->b->dops->raw(h->b->d_dec_state, h->d_bits, n0, n1, lostflag, h->d_pcm, h->d_status, (hipStream_t)0) != hipSuccess) return -1;
    // status + decoded packet in one copy, one synchronisation
    if (hipMemcpyAsync(h->h_blk, h->d_blk, SOLO_SINGLE_PCM_OFF + (size_t)ns * 2, hipMemcpyDeviceToHost, (hipStream_t)0) != hipSuccess) return -1;
    if (hipStreamSynchronize((hipStream_t)0) != hipSuccess) return -1;
    int32_t ret = 0;
    memcpy(&ret, h->h_blk, 4);
    // the reference rewrites the caller's nBytes[] with the low-band lengths (AGR_BWE_decode_frame_FIX.c:150-169)
    int32_t nb0 = (lostflag == 2) ? n0 : n0 - hbb;
    int32_t nb1 = n1 ? n1 - hbb : 0;
    nBytes[0] = (int16_t)(nb0 - nb1);
    nBytes[1] = (int16_t)nb1;
    // like the reference, *nSamplesOut is always written (AGR_BWE_SDK_API.c:277); on a decoder error the PCM buffer is left
    // untouched (the reference leaves whatever its aborted synthesis produced there, which is not defined by its inputs)
    *nSamplesOut = (int16_t)ns;
    if (ret < 0) return ret;
    memcpy(pcm, h->h_blk + SOLO_SINGLE_PCM_OFF, (size_t)ns * 2);
    return 0;
}

int32_t AGR_Sate_Decoder_Uninit(void* st) {
    if (!st) return -1;
    single_free((solo_single*)st);
    return 0;
}

// Conformance probes (tests only; device pointers, default stream, synchronous): the L0 vocabulary of solo_fix.h evaluated by the
// gfx950 build, element-wise; and SKP_Silk_sum_sqr_shift in its wave-cooperative form over `rows` rows of `len` <= 1024 samples.
int32_t solo_debug_l0(int32_t op, int32_t n, const int32_t* d_a, const int32_t* d_b, const int32_t* d_c, int32_t* d_out) {
    if (n <= 0 || !d_a || !d_b || !d_c || !d_out) return -1;
    hipLaunchKernelGGL(solo_l0_probe_kernel, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)0, op, n, d_a, d_b, d_c, d_out);
    SOLO_CHECK(hipGetLastError());
    SOLO_CHECK(hipDeviceSynchronize());
    return 0;
}
int32_t solo_debug_sum_sqr_shift(const int16_t* d_x, int32_t rows, int32_t len, int32_t stride, int32_t odd_start, int32_t* d_energy, int32_t* d_shift) {
    if (rows <= 0 || len <= 0 || len > 1024 || !d_x || !d_energy || !d_shift) return -1;
    hipLaunchKernelGGL(solo_sum_sqr_probe_kernel, dim3(rows), dim3(64), 0, (hipStream_t)0, d_x, len, stride, odd_start, d_energy, d_shift);
    SOLO_CHECK(hipGetLastError());
    SOLO_CHECK(hipDeviceSynchronize());
    return 0;
}

// The lane-crossing vocabulary of solo_wave.h (solo_waveops_probe_kernel above): n_vec vectors of 64 words in d_v and in d_aux, one
// wavefront each, waves_per_block (1 or 4; mode 2, the workgroup vocabulary: 4) of them per workgroup; d_out = int32 [n_vec][rows][64].  Returns `rows` of the mode (also
// for n_vec == 0, which launches nothing: how a caller sizes d_out).
int32_t solo_debug_waveops(int32_t mode, int32_t n_vec, int32_t waves_per_block, const int32_t* d_v, const int32_t* d_aux, int32_t* d_out) {
    if (mode < 0 || mode > 2 || n_vec < 0 || (waves_per_block != 1 && waves_per_block != 4) || (mode == 2 && waves_per_block != 4)) return -1;
    const int32_t rows = mode == 0 ? SOLO_WAVEOPS_ROWS0 : (mode == 1 ? SOLO_WAVEOPS_ROWS1 : SOLO_WAVEOPS_ROWS2);
    if (n_vec == 0) return rows;
    if (!d_v || !d_aux || !d_out) return -1;
    hipLaunchKernelGGL(solo_waveops_probe_kernel, dim3((n_vec + waves_per_block - 1) / waves_per_block), dim3(64 * waves_per_block), 0, (hipStream_t)0,
                       mode, n_vec, waves_per_block, d_v, d_aux, d_out);
    SOLO_CHECK(hipGetLastError());
    SOLO_CHECK(hipDeviceSynchronize());
    return rows;
}

// Stage probes of the decoder (tests/test_dec_stages.py): ONE of the two kernels of the batch path alone, through the launch table of the rate's
// build (samplerate 16000 / 32000), on streams freshly initialised with (useMDIndex, joint, frames_per_packet); HOST pointers, default stream,
// synchronous.  h_bits [n_streams][n_packets][slot_bytes], h_nbytes int16 [n_streams][n_packets][2], h_recv uint8 [n_streams][n_packets] (may be
// NULL: both descriptions of every packet arrived) as solo_batch_decode takes them; `chunk` > 0 walks the packets in launches of `chunk`
// packets with the pipeline's p0 / pc addressing, 0 is one launch.
static const solo_dec_ops* debug_dec_ops(int32_t samplerate) { return samplerate == 16000 ? solo_nb_dec_ops() : (samplerate == 32000 ? solo_wb_dec_ops() : NULL); }
static bool debug_dec_args(const solo_dec_ops* ops, int32_t fpp, int32_t n_streams, int32_t n_packets, int32_t chunk, int32_t slot_bytes) {
    return ops && (fpp == 1 || fpp == 2) && n_streams > 0 && n_packets > 0 && (long long)n_streams * n_packets <= (1 << 16) && chunk >= 0 && slot_bytes > 0 &&
           slot_bytes <= 4096;
}
// The extraction step ALONE (ops->extract: the list kernel, when h_recv is given, and solo_dec_extract_kernel): h_recs =
// SxExtracted[n_streams][n_packets][2], every record of a launch zeroed before it; h_counts (may be NULL) int32 [launches]: the number of
// description slots that carry bytes as the list kernel counted them (-1 without h_recv: no list).  Returns the size of an SxExtracted record;
// n_streams == 0 launches nothing and only returns it.
int32_t solo_debug_dec_extract(int32_t samplerate, int32_t useMDIndex, int32_t joint, int32_t frames_per_packet, int32_t n_streams, int32_t n_packets,
                               int32_t chunk, int32_t slot_bytes, const uint8_t* h_bits, const int16_t* h_nbytes, const uint8_t* h_recv, void* h_recs,
                               int32_t* h_counts) {
    const solo_dec_ops* ops = debug_dec_ops(samplerate);
    if (!ops) return -1;
    const size_t rec = (ops->extracted_bytes - 2 * sizeof(uint32_t)) / 2;
    if (n_streams == 0) return (int32_t)rec;
    if (!debug_dec_args(ops, frames_per_packet, n_streams, n_packets, chunk, slot_bytes) || !h_bits || !h_nbytes || !h_recs) return -1;
    const size_t np = (size_t)n_streams * n_packets, sz_bits = np * (size_t)slot_bytes, sz_nb = np * 2 * sizeof(int16_t);
    const int cp = chunk > 0 && chunk < n_packets ? chunk : n_packets;
    const size_t lanes = (size_t)n_streams * cp * 2, sz_recs = (size_t)n_streams * cp * ops->extracted_bytes + 256;
    void *st = NULL, *d_bits = NULL, *d_nb = NULL, *d_recv = NULL, *d_recs = NULL;
    int32_t rc = -1;
    bool ok = hipMalloc(&st, ops->state_bytes * (size_t)n_streams) == hipSuccess && hipMalloc(&d_bits, sz_bits) == hipSuccess && hipMalloc(&d_nb, sz_nb) == hipSuccess &&
              hipMalloc(&d_recs, sz_recs) == hipSuccess && (!h_recv || hipMalloc(&d_recv, np) == hipSuccess) &&
              ops->init(st, n_streams, (joint ? 1 : 0) | (frames_per_packet == 1 ? 2 : 0), useMDIndex, (hipStream_t)0) == hipSuccess &&
              hipMemcpy(d_bits, h_bits, sz_bits, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(d_nb, h_nbytes, sz_nb, hipMemcpyHostToDevice) == hipSuccess &&
              (!h_recv || hipMemcpy(d_recv, h_recv, np, hipMemcpyHostToDevice) == hipSuccess);
    int launch = 0;
    for (int p0 = 0; ok && p0 < n_packets; p0 += cp, launch++) {
        const int pc = p0 + cp <= n_packets ? cp : n_packets - p0;
        ok = hipMemset(d_recs, 0, sz_recs) == hipSuccess &&
             ops->extract(st, (const uint8_t*)d_bits, (const int16_t*)d_nb, (const uint8_t*)d_recv, n_streams, n_packets, p0, pc, slot_bytes, d_recs, NULL, NULL,
                          (hipStream_t)0) == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
             // device rows [stream][pc][2] -> host rows [stream][n_packets][2]
             hipMemcpy2D((char*)h_recs + (size_t)p0 * 2 * rec, (size_t)n_packets * 2 * rec, d_recs, (size_t)pc * 2 * rec, (size_t)pc * 2 * rec, (size_t)n_streams,
                         hipMemcpyDeviceToHost) == hipSuccess;
        if (ok && h_counts) {
            h_counts[launch] = -1;
            // (the list and its count lie behind the records of THIS launch: solo_dec_launch_extract)
            if (h_recv) ok = hipMemcpy(&h_counts[launch], (char*)d_recs + (size_t)n_streams * pc * 2 * rec + (size_t)n_streams * pc * 2 * sizeof(uint32_t), sizeof(int32_t),
                                       hipMemcpyDeviceToHost) == hipSuccess;
        }
    }
    (void)lanes;
    if (ok) rc = (int32_t)rec;
    (void)hipFree(st); (void)hipFree(d_bits); (void)hipFree(d_nb); (void)hipFree(d_recv); (void)hipFree(d_recs);
    return rc;
}
// The decoder proper ALONE: with h_recs (SxExtracted[n_streams][n_packets][2]: the extract probe's, or packed by the caller from the reference's
// symbols) ops->synth consumes them; with h_recs == NULL the single kernel ops->decode reads the symbols itself.  After EVERY launch the PCM of
// its packets goes to h_pcm int16 [n_streams][n_packets][samples of a packet], the status word to h_status int32 [launches][n_streams] and the
// first state_bytes bytes of every stream record -- its SxDecState -- to h_state [launches][n_streams][state_bytes] (may be NULL).  Returns the
// size of an SxExtracted record.
int32_t solo_debug_dec_synth(int32_t samplerate, int32_t useMDIndex, int32_t joint, int32_t frames_per_packet, int32_t n_streams, int32_t n_packets,
                             int32_t chunk, int32_t slot_bytes, const uint8_t* h_bits, const int16_t* h_nbytes, const uint8_t* h_recv, const void* h_recs,
                             int16_t* h_pcm, int32_t* h_status, void* h_state, int32_t state_bytes) {
    const solo_dec_ops* ops = debug_dec_ops(samplerate);
    if (!debug_dec_args(ops, frames_per_packet, n_streams, n_packets, chunk, slot_bytes) || !h_bits || !h_nbytes || !h_pcm || !h_status || state_bytes < 0 ||
        (size_t)state_bytes > ops->state_bytes || (h_state == NULL) != (state_bytes == 0))
        return -1;
    const size_t rec = (ops->extracted_bytes - 2 * sizeof(uint32_t)) / 2;
    const size_t np = (size_t)n_streams * n_packets, sz_bits = np * (size_t)slot_bytes, sz_nb = np * 2 * sizeof(int16_t);
    const size_t samples = (size_t)(ops->packet_samples / 2 * frames_per_packet), sz_pcm = np * samples * sizeof(int16_t), sz_st = (size_t)n_streams * sizeof(int32_t);
    const int cp = chunk > 0 && chunk < n_packets ? chunk : n_packets;
    const size_t sz_recs = (size_t)n_streams * cp * ops->extracted_bytes + 256;
    void *st = NULL, *d_bits = NULL, *d_nb = NULL, *d_recv = NULL, *d_recs = NULL, *d_pcm = NULL, *d_status = NULL;
    int32_t rc = -1;
    bool ok = hipMalloc(&st, ops->state_bytes * (size_t)n_streams) == hipSuccess && hipMalloc(&d_bits, sz_bits) == hipSuccess && hipMalloc(&d_nb, sz_nb) == hipSuccess &&
              hipMalloc(&d_pcm, sz_pcm) == hipSuccess && hipMalloc(&d_status, sz_st) == hipSuccess && hipMalloc(&d_recv, np) == hipSuccess &&
              (!h_recs || hipMalloc(&d_recs, sz_recs) == hipSuccess) && hipMemset(d_pcm, 0, sz_pcm) == hipSuccess && hipMemset(d_status, 0xFF, sz_st) == hipSuccess &&
              ops->init(st, n_streams, (joint ? 1 : 0) | (frames_per_packet == 1 ? 2 : 0), useMDIndex, (hipStream_t)0) == hipSuccess;
    if (ok && h_recs) {
        ok = hipMemcpy(d_bits, h_bits, sz_bits, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(d_nb, h_nbytes, sz_nb, hipMemcpyHostToDevice) == hipSuccess &&
             (h_recv ? hipMemcpy(d_recv, h_recv, np, hipMemcpyHostToDevice) : hipMemset(d_recv, 3, np)) == hipSuccess;
    }
    int launch = 0;
    for (int p0 = 0; ok && p0 < n_packets; p0 += cp, launch++) {
        const int pc = p0 + cp <= n_packets ? cp : n_packets - p0;
        if (h_recs) {
            // host rows [stream][n_packets][2] -> device rows [stream][pc][2]
            ok = hipMemcpy2D(d_recs, (size_t)pc * 2 * rec, (const char*)h_recs + (size_t)p0 * 2 * rec, (size_t)n_packets * 2 * rec, (size_t)pc * 2 * rec, (size_t)n_streams,
                             hipMemcpyHostToDevice) == hipSuccess &&
                 ops->synth(st, (const uint8_t*)d_bits, (const int16_t*)d_nb, (const uint8_t*)d_recv, n_streams, n_packets, p0, pc, slot_bytes, d_recs, (int16_t*)d_pcm,
                            (int32_t*)d_status, NULL, NULL, (hipStream_t)0) == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
                 hipMemcpy2D(h_pcm + (size_t)p0 * samples, (size_t)n_packets * samples * 2, (const int16_t*)d_pcm + (size_t)p0 * samples, (size_t)n_packets * samples * 2,
                             (size_t)pc * samples * 2, (size_t)n_streams, hipMemcpyDeviceToHost) == hipSuccess;
        } else {
            // the single kernel has no p0: the launch's packets are handed to it as a call of their own, rows [stream][pc]
            ok = hipMemcpy2D(d_bits, (size_t)pc * slot_bytes, h_bits + (size_t)p0 * slot_bytes, (size_t)n_packets * slot_bytes, (size_t)pc * slot_bytes, (size_t)n_streams,
                             hipMemcpyHostToDevice) == hipSuccess &&
                 hipMemcpy2D(d_nb, (size_t)pc * 4, h_nbytes + (size_t)p0 * 2, (size_t)n_packets * 4, (size_t)pc * 4, (size_t)n_streams, hipMemcpyHostToDevice) == hipSuccess &&
                 (h_recv ? hipMemcpy2D(d_recv, (size_t)pc, h_recv + p0, (size_t)n_packets, (size_t)pc, (size_t)n_streams, hipMemcpyHostToDevice) : hipMemset(d_recv, 3, np)) ==
                     hipSuccess &&
                 ops->decode(st, (const uint8_t*)d_bits, (const int16_t*)d_nb, (const uint8_t*)d_recv, n_streams, pc, slot_bytes, (int16_t*)d_pcm, (int32_t*)d_status, NULL,
                             NULL, (hipStream_t)0) == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
                 hipMemcpy2D(h_pcm + (size_t)p0 * samples, (size_t)n_packets * samples * 2, d_pcm, (size_t)pc * samples * 2, (size_t)pc * samples * 2, (size_t)n_streams,
                             hipMemcpyDeviceToHost) == hipSuccess;
        }
        ok = ok && hipMemcpy(h_status + (size_t)launch * n_streams, d_status, sz_st, hipMemcpyDeviceToHost) == hipSuccess &&
             (!h_state || hipMemcpy2D((char*)h_state + (size_t)launch * n_streams * state_bytes, (size_t)state_bytes, st, ops->state_bytes, (size_t)state_bytes,
                                      (size_t)n_streams, hipMemcpyDeviceToHost) == hipSuccess);
    }
    if (ok) rc = (int32_t)rec;
    (void)hipFree(st); (void)hipFree(d_bits); (void)hipFree(d_nb); (void)hipFree(d_recv); (void)hipFree(d_recs); (void)hipFree(d_pcm); (void)hipFree(d_status);
    return rc;
}

#ifdef SOLO_WITH_ENCODER
// Stage probes of the encoder (tests/test_nsq_taps.py, tests/test_enc_stages.py): each runs ONE of the three stages of the launch-per-chunk schedule
// alone, through the launch table of the rate's build, on freshly initialised streams; HOST pointers; default stream; synchronous.  `samplerate`
// 16000 / 32000 picks the table; silk_rate_bps, useMDIndex, joint, dtx, frames_per_packet are the arguments of its `init`.
static const solo_enc_ops* debug_enc_ops(int32_t samplerate) { return samplerate == 16000 ? solo_nb_enc_ops() : (samplerate == 32000 ? solo_wb_enc_ops() : NULL); }
static bool debug_enc_args(const solo_enc_ops* ops, int32_t fpp, int32_t n_streams, int32_t n_packets) {
    return ops && (fpp == 1 || fpp == 2) && n_streams > 0 && n_packets > 0 && (long long)n_streams * n_packets <= (1 << 20);
}
// The quantiser kernel ALONE: h_in = SxNsqIn[n_streams][n_packets][2] as recorded from the reference's SKP_Silk_NSQ_del_dec calls (or as the
// analysis probe left them), h_out = SxNsqOut[n_streams][n_packets][2].  Returns the output record size.
int32_t solo_debug_nsq_ex(int32_t samplerate, int32_t silk_rate_bps, int32_t useMDIndex, int32_t joint, int32_t dtx, int32_t frames_per_packet,
                          int32_t n_streams, int32_t n_packets, const void* h_in, void* h_out) {
    const solo_enc_ops* ops = debug_enc_ops(samplerate);
    if (!debug_enc_args(ops, frames_per_packet, n_streams, n_packets) || !h_in || !h_out) return -1;
    const size_t sz_in = (size_t)n_streams * n_packets * 2 * ops->nsq_in_bytes, sz_out = (size_t)n_streams * n_packets * 2 * ops->nsq_out_bytes;
    void *st = NULL, *d_in = NULL, *d_out = NULL, *ring = NULL;
    int32_t rc = -1;
    if (hipMalloc(&st, ops->state_bytes * (size_t)n_streams) == hipSuccess && hipMalloc(&d_in, sz_in) == hipSuccess && hipMalloc(&d_out, sz_out) == hipSuccess &&
        hipMalloc(&ring, ops->nsq_ring_bytes(n_streams)) == hipSuccess && hipMemset(d_out, 0, sz_out) == hipSuccess &&
        ops->init(st, n_streams, silk_rate_bps, useMDIndex, joint, dtx, frames_per_packet, (hipStream_t)0) == hipSuccess &&
        hipMemcpy(d_in, h_in, sz_in, hipMemcpyHostToDevice) == hipSuccess &&
        ops->nsq(st, d_in, d_out, n_streams, n_packets, 0, n_packets, NULL, ring, NULL, NULL, NULL) == 0 && hipDeviceSynchronize() == hipSuccess &&
        hipMemcpy(h_out, d_out, sz_out, hipMemcpyDeviceToHost) == hipSuccess)
        rc = (int32_t)ops->nsq_out_bytes;                       // (the caller checks its idea of the record size)
    (void)hipFree(st); (void)hipFree(d_in); (void)hipFree(d_out); (void)hipFree(ring);
    return rc;
}
int32_t solo_debug_nsq(int32_t n_streams, int32_t n_packets, const void* h_in, void* h_out) {
    return solo_debug_nsq_ex(16000, 12000, 0, 0, 0, 2, n_streams, n_packets, h_in, h_out);
}
// The analysis kernel ALONE: h_pcm = int16 [n_streams][n_packets][packet samples] -> h_nsq_in = SxNsqIn[n_streams][n_packets][2], h_code_in =
// SxCodeIn[n_streams][n_packets], by ops->analysis with the pipeline's p0 / pc addressing: chunk > 0 walks the packets in launches of `chunk`
// packets (the compact state goes through the stream record between two launches), 0 is one launch.  h_sizes (may be NULL) receives
// {nsq_in_bytes, nsq_out_bytes, code_in_bytes, samples of a 40 ms packet, front_waves} of the table; n_streams == 0 launches nothing
// and only fills it.  Returns the size of an SxNsqIn record.
int32_t solo_debug_analysis(int32_t samplerate, int32_t silk_rate_bps, int32_t useMDIndex, int32_t joint, int32_t dtx, int32_t frames_per_packet,
                            int32_t n_streams, int32_t n_packets, int32_t chunk, const int16_t* h_pcm, void* h_nsq_in, void* h_code_in, int32_t* h_sizes) {
    const solo_enc_ops* ops = debug_enc_ops(samplerate);
    if (!ops) return -1;
    if (h_sizes) {
        h_sizes[0] = (int32_t)ops->nsq_in_bytes; h_sizes[1] = (int32_t)ops->nsq_out_bytes; h_sizes[2] = (int32_t)ops->code_in_bytes;
        h_sizes[3] = ops->packet_samples; h_sizes[4] = ops->front_waves;
    }
    if (n_streams == 0) return (int32_t)ops->nsq_in_bytes;
    if (!debug_enc_args(ops, frames_per_packet, n_streams, n_packets) || chunk < 0 || !h_pcm || !h_nsq_in || !h_code_in) return -1;
    const size_t np = (size_t)n_streams * n_packets;
    const size_t sz_pcm = np * (size_t)(ops->packet_samples / 2 * frames_per_packet) * 2, sz_in = np * 2 * ops->nsq_in_bytes, sz_code = np * ops->code_in_bytes;
    void *st = NULL, *d_pcm = NULL, *d_in = NULL, *d_code = NULL;
    int32_t rc = -1;
    const int cp = chunk > 0 ? chunk : n_packets;
    bool ok = hipMalloc(&st, ops->state_bytes * (size_t)n_streams) == hipSuccess && hipMalloc(&d_pcm, sz_pcm) == hipSuccess && hipMalloc(&d_in, sz_in) == hipSuccess &&
              hipMalloc(&d_code, sz_code) == hipSuccess && hipMemset(d_in, 0, sz_in) == hipSuccess && hipMemset(d_code, 0, sz_code) == hipSuccess &&
              ops->init(st, n_streams, silk_rate_bps, useMDIndex, joint, dtx, frames_per_packet, (hipStream_t)0) == hipSuccess &&
              hipMemcpy(d_pcm, h_pcm, sz_pcm, hipMemcpyHostToDevice) == hipSuccess;
    for (int p0 = 0; ok && p0 < n_packets; p0 += cp)
        ok = ops->analysis(st, (const int16_t*)d_pcm, n_streams, n_packets, p0, p0 + cp <= n_packets ? cp : n_packets - p0, d_in, d_code, NULL, NULL, (hipStream_t)0) == hipSuccess;
    if (ok && hipDeviceSynchronize() == hipSuccess && hipMemcpy(h_nsq_in, d_in, sz_in, hipMemcpyDeviceToHost) == hipSuccess &&
        hipMemcpy(h_code_in, d_code, sz_code, hipMemcpyDeviceToHost) == hipSuccess)
        rc = (int32_t)ops->nsq_in_bytes;
    (void)hipFree(st); (void)hipFree(d_pcm); (void)hipFree(d_in); (void)hipFree(d_code);
    return rc;
}
// The coding stage ALONE (high band, range coder, payload assembly): h_code_in = SxCodeIn[n_streams][n_packets], h_nsq_out =
// SxNsqOut[n_streams][n_packets][2] -> h_bits [n_streams][n_packets][slot_bytes], h_nbytes int16 [n_streams][n_packets][2], h_status int32
// [n_streams], by ops->coding on a scratch of ops->rc_scratch_bytes, in launches of `chunk` packets (0: one).  Of the stream record the stage
// reads what `init` sets (useMDIndex, useDTX, hb_joint, fpp) and owns the high-band history, which it alone writes: nothing that the analysis
// stage leaves per packet, so freshly initialised streams are all it needs.  Returns the size of an SxCodeIn record.
int32_t solo_debug_coding(int32_t samplerate, int32_t silk_rate_bps, int32_t useMDIndex, int32_t joint, int32_t dtx, int32_t frames_per_packet,
                          int32_t n_streams, int32_t n_packets, int32_t chunk, int32_t slot_bytes, const void* h_code_in, const void* h_nsq_out,
                          uint8_t* h_bits, int16_t* h_nbytes, int32_t* h_status) {
    const solo_enc_ops* ops = debug_enc_ops(samplerate);
    if (!debug_enc_args(ops, frames_per_packet, n_streams, n_packets) || chunk < 0 || slot_bytes <= 0 || slot_bytes > 4096 || !h_code_in || !h_nsq_out || !h_bits ||
        !h_nbytes || !h_status)
        return -1;
    const size_t np = (size_t)n_streams * n_packets;
    const size_t sz_code = np * ops->code_in_bytes, sz_out = np * 2 * ops->nsq_out_bytes, sz_bits = np * (size_t)slot_bytes, sz_nb = np * 2 * sizeof(int16_t),
                 sz_st = (size_t)n_streams * sizeof(int32_t);
    const int cp = chunk > 0 && chunk < n_packets ? chunk : n_packets;
    void *st = NULL, *d_code = NULL, *d_out = NULL, *d_bits = NULL, *d_nb = NULL, *d_status = NULL, *scratch = NULL;
    int32_t rc = -1;
    bool ok = hipMalloc(&st, ops->state_bytes * (size_t)n_streams) == hipSuccess && hipMalloc(&d_code, sz_code) == hipSuccess && hipMalloc(&d_out, sz_out) == hipSuccess &&
              hipMalloc(&d_bits, sz_bits) == hipSuccess && hipMalloc(&d_nb, sz_nb) == hipSuccess && hipMalloc(&d_status, sz_st) == hipSuccess &&
              hipMalloc(&scratch, ops->rc_scratch_bytes(n_streams, cp)) == hipSuccess && hipMemset(d_bits, 0, sz_bits) == hipSuccess &&
              hipMemset(d_nb, 0xFF, sz_nb) == hipSuccess && hipMemset(d_status, 0xFF, sz_st) == hipSuccess &&
              ops->init(st, n_streams, silk_rate_bps, useMDIndex, joint, dtx, frames_per_packet, (hipStream_t)0) == hipSuccess &&
              hipMemcpy(d_code, h_code_in, sz_code, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(d_out, h_nsq_out, sz_out, hipMemcpyHostToDevice) == hipSuccess;
    for (int p0 = 0; ok && p0 < n_packets; p0 += cp)
        ok = ops->coding(st, d_code, d_out, n_streams, n_packets, p0, p0 + cp <= n_packets ? cp : n_packets - p0, slot_bytes, (uint8_t*)d_bits, (int16_t*)d_nb,
                         (int32_t*)d_status, scratch, NULL, NULL, (hipStream_t)0) == hipSuccess;
    if (ok && hipDeviceSynchronize() == hipSuccess && hipMemcpy(h_bits, d_bits, sz_bits, hipMemcpyDeviceToHost) == hipSuccess &&
        hipMemcpy(h_nbytes, d_nb, sz_nb, hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(h_status, d_status, sz_st, hipMemcpyDeviceToHost) == hipSuccess)
        rc = (int32_t)ops->code_in_bytes;
    (void)hipFree(st); (void)hipFree(d_code); (void)hipFree(d_out); (void)hipFree(d_bits); (void)hipFree(d_nb); (void)hipFree(d_status); (void)hipFree(scratch);
    return rc;
}
#endif

#if defined(SX_PROF)
// debug builds only: read (and clear) the per-section cycle counters of the decoder kernels (tools/prof_dec.py; the encoder kernels'
// counters live in their own translation unit: solo_debug_prof_enc, solo_enc_k.hip)
int32_t solo_debug_prof(unsigned long long* out64, int32_t reset) {
    if (hipMemcpyFromSymbol(out64, HIP_SYMBOL(g_sx_prof), 64 * sizeof(unsigned long long)) != hipSuccess) return -1;
    if (reset) {
        unsigned long long z[64] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_sx_prof), z, sizeof(z)) != hipSuccess) return -1;
    }
    return 0;
}
#endif

#if defined(SX_STOPS)
// debug builds only (tools/debug/analysis_sections.py dec): where the decoder's waves of the next launches end (0: nowhere), and how often
// each site was passed by the launches that ran through
int32_t solo_debug_stop_dec(int32_t site_hit) { return hipMemcpyToSymbol(HIP_SYMBOL(g_sx_stop), &site_hit, sizeof(site_hit)) == hipSuccess ? 0 : -1; }
int32_t solo_debug_site_hits_dec(unsigned long long* out64, int32_t reset) {
    if (hipMemcpyFromSymbol(out64, HIP_SYMBOL(g_sx_site_hits), 128 * sizeof(unsigned long long)) != hipSuccess) return -1;
    if (reset) {
        unsigned long long z[128] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_sx_site_hits), z, sizeof(z)) != hipSuccess) return -1;
    }
    return 0;
}
#endif

}  // extern "C"

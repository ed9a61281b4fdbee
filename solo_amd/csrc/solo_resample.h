// solo_resample.h -- PCM rate conversion between handles of different rates and towards 8 / 48 kHz endpoints (solo_resample,
// include/solo_mi355x.h): the reference's own fixed-point resampler (SKP_Silk_resampler_init / SKP_Silk_resampler,
// JC1_SDK_SRC_ARM/src/libSATECodec/SKP_Silk_resampler*.c), bit for bit, with its stream state.  Rate independent, compiled once.
//
//     kind 0  down (48->16, 48->32, 32->16, 16->8)   private_down_FIR: AR2 (output in Q8, 32 bits) + 12-tap FIR over the Q8 signal
//     kind 1  up 2x (16->32, 8->16)                  private_up2_HQ_wrapper: two all-pass pairs + the notch that couples them
//     kind 2  up 3x (16->48)                         private_IIR_FIR: up2_HQ, then the 6-tap interpolation over the 144-phase table
//     kind 3  up 1.5x (32->48)                       private_IIR_FIR with the one-section up2 (fs_in > 24000)
//
// The reference cuts its input into batches of 10 ms (batchSize = fs_in / 100) and restarts the interpolation index at 0 in every
// batch, so the kernel walks the same batches: P packets in one call are P calls of one packet, and a packet is whole batches.
//
// The state record of a row is the first 96 bytes of the reference's struct: sIIR[6], sFIR[16], sDown2[2], 32 bits each.  Kind 0 keeps
// 12 words of Q8 history in sFIR[0..12).  Kinds 2 and 3 keep their SIX int16 of history in sFIR[0..3): the reference copies
// 6 * sizeof(int32) bytes to and from an int16 buffer (private_IIR_FIR.c:79,101,108), so six more int16 travel with them -- they are read
// from beyond the batch's last sample and overwritten by the next batch's first samples before anything reads them.  This kernel
// carries the six that matter and leaves sFIR[3..6) as it finds it (zero after a reset).
//
// One workgroup = ONE wavefront = SX_RS_ROWS rows.  Per batch, with the rows' buffers in LDS (row stride an odd number of words, so that
// lanes on different rows hit different banks):
//     A  load       all lanes: the rows' batch of input, 16 bytes per lane, coalesced along each row, into the row's staging area
//     B  recur      lanes 0 .. rows-1, one row each: the serial part (AR2, or the all-pass sections and the notch), input from the staging
//                   area, output into the row's `mid` buffer behind its history (int32 Q8 for kind 0, int16 otherwise).  32-bit wrapping
//                   arithmetic, truncating multiplies: not re-associable.  The two all-pass chains of up2_HQ meet in the notch at every
//                   sample (its state S[4], S[5] crosses over), so one lane runs both: they interleave as independent instructions.
//     C  interp     all lanes, one OUTPUT SAMPLE per lane and step (neighbouring lanes read neighbouring words of `mid`): the FIR /
//                   the table interpolation / the copy of kind 1, saturated, into the staging area (its input is used up)
//     D  store      all lanes: the staging area to memory, 16 bytes per lane, coalesced; the history moves to the front of `mid`
// The state record is read once per launch (sIIR stays in the recurrence lane's registers) and written once.
//
// Everything outside the kernels compiles for the host with the 1-lane forms of solo_wave.h (tests/test_resample_model.py builds
// sx_rs_host through tests/resample_host.cpp and compares it with the fixture recorded from the compiled reference).
#pragma once
#include "solo_wave.h"
#include "solo_stream_ctl.h"
#include "../../include/solo_mi355x.h"

#if !defined(SOLO_TAB)
#if defined(__HIPCC__)
#define SOLO_TAB static __device__ const
#else
#define SOLO_TAB static const
#endif
#endif
#include "solo_resample_tables.inc"

#define SX_RS_ROWS 16                                       // rows of a workgroup (DESIGN.md section 10 has the LDS and occupancy arithmetic)
#define SX_RS_STATE_WORDS 24                                // sIIR[6] | sFIR[16] | sDown2[2]
#define SX_RS_MAX_BATCH 480                                 // 10 ms at 48 kHz
#define SX_RS_DOWN_FIR 12                                   // taps of kind 0 = words of its history
#define SX_RS_UP_HIST 6                                     // int16 of history of kinds 2 and 3

struct SxRsCfg {
    i32 kind;                   // 0 .. 3 above
    i32 n_in, n_out;            // samples of a batch, in and out
    i32 inc_Q16;                // invRatio_Q16: step of the interpolation index (kinds 0, 2, 3)
    i32 fracs;                  // kind 0: FIR_Fracs (1 or 2)
    i32 coefs;                  // kind 0: 0 = 1:3, 1 = 2:3, 2 = 1:2
    i32 mid_words, row_words;   // LDS words of a row's mid buffer (history included), and of the whole row (odd)
};
typedef solo_resample_count_t SxRsCount;

static inline bool sx_rs_rate_ok(i32 fs) { return fs == 8000 || fs == 16000 || fs == 32000 || fs == 48000; }
// The conversions of this library -> false for every other pair.  invRatio_Q16 as SKP_Silk_resampler_init computes it
// (SKP_Silk_resampler.c:243-247): floor((fs_in << (14 + up2)) / fs_out) << 2, then raised until invRatio * fs_out >= fs_in << up2 in Q16.
static inline bool sx_rs_config(i32 fs_in, i32 fs_out, SxRsCfg* c) {
    if (!sx_rs_rate_ok(fs_in) || !sx_rs_rate_ok(fs_out)) return false;
    i32 up2 = 0;
    c->fracs = 1; c->coefs = 0;
    if (fs_out * 3 == fs_in) { c->kind = 0; c->coefs = 0; }
    else if (fs_out * 3 == fs_in * 2) { c->kind = 0; c->coefs = 1; c->fracs = 2; }
    else if (fs_out * 2 == fs_in) { c->kind = 0; c->coefs = 2; }
    else if (fs_out == fs_in * 2) c->kind = 1;
    else if (fs_out == fs_in * 3) { c->kind = 2; up2 = 1; }
    else if (fs_out * 2 == fs_in * 3) { c->kind = 3; up2 = 1; }
    else return false;
    if (c->kind == 2 && fs_in > 24000) return false;        // (no such pair among the four rates; kind 2 IS the fs_in <= 24000 branch)
    c->n_in = fs_in / 100;
    c->n_out = fs_out / 100;
    i32 inv = (i32)((((i64)fs_in << (14 + up2)) / fs_out) << 2);
    while (sx_smulww(inv, fs_out) < (fs_in << up2)) inv++;
    c->inc_Q16 = inv;
    c->mid_words = c->kind == 0 ? SX_RS_DOWN_FIR + c->n_in : SX_RS_UP_HIST / 2 + c->n_in;
    c->row_words = (c->mid_words + (c->n_in > c->n_out ? c->n_in : c->n_out) / 2) | 1;
    return true;
}
// output samples of in_samples input samples; -1 unless in_samples is a positive multiple of a batch
static inline i32 sx_rs_out_samples(const SxRsCfg& c, i32 in_samples) {
    if (in_samples <= 0 || in_samples % c.n_in) return -1;
    return in_samples / c.n_in * c.n_out;
}
// what the host checks of a call before it enqueues anything
static inline bool sx_rs_call_ok(const SxRsCfg& c, i32 n_rows, i32 n, i32 n_packets, i32 in_samples, const void* in, const void* out) {
    if (!in || !out || n <= 0 || n > n_rows || n_packets <= 0) return false;
    const i32 outs = sx_rs_out_samples(c, in_samples);
    if (outs < 0) return false;
    const i64 e_in = (i64)n * (i64)n_packets * (i64)in_samples, e_out = (i64)n * (i64)n_packets * (i64)outs;
    if (e_in >= ((i64)1 << 31) || e_out >= ((i64)1 << 31)) return false;
    const uintptr_t a = (uintptr_t)in, b = (uintptr_t)out;
    if ((a & 15) || (b & 15)) return false;
    return !(a < b + (uintptr_t)e_out * 2 && b < a + (uintptr_t)e_in * 2);
}
// (the name the host build of tests/resample_host.cpp asks the host-list rule by)
static inline bool sx_rs_list_ok(const i32* rows, i32 n, i32 n_rows) { return sx_list_ok(rows, n, n_rows); }

struct alignas(16) SxRsX8 { u32 w[4]; };                    // what one lane loads and stores: 8 samples

struct SxRsArgs {
    SxRsCfg c;
    const i16* in; i16* out;        // [n][batches * n_in], [n][batches * n_out]
    i32* state;                     // [n_rows][SX_RS_STATE_WORDS]
    const i32* map;                 // compact position -> row of the object, or NULL = the identity
    i32 n, batches;                 // rows of the call, batches per row (packets x batches of a packet)
};

SX_HD i32 sx_rs_s16(u32 w, int hi) { return (i32)(i16)(hi ? (w >> 16) : (w & 0xFFFFu)); }
SX_HD u32 sx_rs_pack(i32 lo, i32 hi) { return ((u32)lo & 0xFFFFu) | ((u32)hi << 16); }

// ---- B: the serial part of one row and batch.  S: the row's sIIR (registers), in: n_in samples, two per word ----------------------
// SKP_Silk_resampler_private_AR2 (private_AR2.c:52-58): out_Q8 behind the 12 words of history
SX_HD void sx_rs_ar2(i32 (&S)[6], const u32* in, i32* mid, int n_in, const i16* A_Q14) {
    const i32 a0 = sx_pre16(A_Q14[0]), a1 = sx_pre16(A_Q14[1]);
    i32 s0 = S[0], s1 = S[1];
    i32* o = mid + SX_RS_DOWN_FIR;
    u32 x[4] = {in[0], in[1], in[2], in[3]};
    for (int k = 0; k < n_in; k += 8) {
        u32 nx[4] = {0, 0, 0, 0};
        if (k + 8 < n_in) { nx[0] = in[(k >> 1) + 4]; nx[1] = in[(k >> 1) + 5]; nx[2] = in[(k >> 1) + 6]; nx[3] = in[(k >> 1) + 7]; }
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const i32 out32 = sx_add(s0, sx_shl(sx_rs_s16(x[j >> 1], j & 1), 8));
            o[k + j] = out32;
            const i32 t = sx_shl(out32, 2);
            s0 = sx_smlaw_pre(s1, t, a0);
            s1 = sx_smulw_pre(t, a1);
        }
#pragma unroll
        for (int j = 0; j < 4; j++) x[j] = nx[j];
    }
    S[0] = s0; S[1] = s1;
}
// SKP_Silk_resampler_private_up2_HQ (private_up2_HQ.c:59-106): sample k -> int16 6 + 2k and 7 + 2k of mid = word 3 + k
SX_HD void sx_rs_up2_hq(i32 (&S)[6], const u32* in, u32* mid, int n_in) {
    const i32 h00 = sx_pre16(T_rs_up2_hq_0[0]), h01 = sx_pre16(T_rs_up2_hq_0[1]), h10 = sx_pre16(T_rs_up2_hq_1[0]), h11 = sx_pre16(T_rs_up2_hq_1[1]);
    const i32 n0 = sx_pre16(T_rs_up2_hq_notch[0]), n1 = sx_pre16(T_rs_up2_hq_notch[1]), n2 = sx_pre16(T_rs_up2_hq_notch[2]), n3 = sx_pre16(T_rs_up2_hq_notch[3]);
    i32 s0 = S[0], s1 = S[1], s2 = S[2], s3 = S[3], s4 = S[4], s5 = S[5];
    u32* o = mid + SX_RS_UP_HIST / 2;
    u32 x[4] = {in[0], in[1], in[2], in[3]};
    for (int k = 0; k < n_in; k += 8) {
        u32 nx[4] = {0, 0, 0, 0};
        if (k + 8 < n_in) { nx[0] = in[(k >> 1) + 4]; nx[1] = in[(k >> 1) + 5]; nx[2] = in[(k >> 1) + 6]; nx[3] = in[(k >> 1) + 7]; }
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const i32 in32 = sx_shl(sx_rs_s16(x[j >> 1], j & 1), 10);
            // even output sample: two all-pass sections, the notch
            i32 Y = sx_sub(in32, s0);
            i32 X = sx_smulw_pre(Y, h00);
            i32 o1 = sx_add(s0, X);
            s0 = sx_add(in32, X);
            Y = sx_sub(o1, s1);
            X = sx_smlaw_pre(Y, Y, h01);
            i32 o2 = sx_add(s1, X);
            s1 = sx_add(o1, X);
            o2 = sx_smlaw_pre(o2, s5, n2);
            o2 = sx_smlaw_pre(o2, s4, n1);
            o1 = sx_smlaw_pre(o2, s4, n0);
            s5 = sx_sub(o2, s5);
            const i32 even = sx_sat16(sx_smlaw_pre(256, o1, n3) >> 9);
            // odd output sample
            Y = sx_sub(in32, s2);
            X = sx_smulw_pre(Y, h10);
            o1 = sx_add(s2, X);
            s2 = sx_add(in32, X);
            Y = sx_sub(o1, s3);
            X = sx_smlaw_pre(Y, Y, h11);
            o2 = sx_add(s3, X);
            s3 = sx_add(o1, X);
            o2 = sx_smlaw_pre(o2, s4, n2);
            o2 = sx_smlaw_pre(o2, s5, n1);
            o1 = sx_smlaw_pre(o2, s5, n0);
            s4 = sx_sub(o2, s4);
            const i32 odd = sx_sat16(sx_smlaw_pre(256, o1, n3) >> 9);
            o[k + j] = sx_rs_pack(even, odd);
        }
#pragma unroll
        for (int j = 0; j < 4; j++) x[j] = nx[j];
    }
    S[0] = s0; S[1] = s1; S[2] = s2; S[3] = s3; S[4] = s4; S[5] = s5;
}
// SKP_Silk_resampler_up2 (up2.c:54-75): one all-pass section per output phase
SX_HD void sx_rs_up2_lq(i32 (&S)[6], const u32* in, u32* mid, int n_in) {
    const i32 l0 = sx_pre16(T_rs_up2_lq[0]), l1 = sx_pre16(T_rs_up2_lq[1]);
    i32 s0 = S[0], s1 = S[1];
    u32* o = mid + SX_RS_UP_HIST / 2;
    u32 x[4] = {in[0], in[1], in[2], in[3]};
    for (int k = 0; k < n_in; k += 8) {
        u32 nx[4] = {0, 0, 0, 0};
        if (k + 8 < n_in) { nx[0] = in[(k >> 1) + 4]; nx[1] = in[(k >> 1) + 5]; nx[2] = in[(k >> 1) + 6]; nx[3] = in[(k >> 1) + 7]; }
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const i32 in32 = sx_shl(sx_rs_s16(x[j >> 1], j & 1), 10);
            i32 Y = sx_sub(in32, s0);
            i32 X = sx_smulw_pre(Y, l0);
            const i32 even = sx_sat16(sx_rshift_round(sx_add(s0, X), 10));
            s0 = sx_add(in32, X);
            Y = sx_sub(in32, s1);
            X = sx_smlaw_pre(Y, Y, l1);
            const i32 odd = sx_sat16(sx_rshift_round(sx_add(s1, X), 10));
            s1 = sx_add(in32, X);
            o[k + j] = sx_rs_pack(even, odd);
        }
#pragma unroll
        for (int j = 0; j < 4; j++) x[j] = nx[j];
    }
    S[0] = s0; S[1] = s1;
}

// ---- C: output sample j of a batch from the row's mid buffer ------------------------------------------------------------------------
// private_down_FIR.c:45-59 (FIR_Fracs 1: the symmetric form) and :70-95 (the interpolating form); FIR_Coefs = Coefs + 2
SX_HD i32 sx_rs_down_fir(const i32* mid, int j, const SxRsCfg& c, const i16* coefs) {
    const i32 idx = j * c.inc_Q16;
    const i32* b = mid + (idx >> 16);
    const i16* f = coefs + 2;
    i32 r;
    if (c.fracs == 1) {
        r = sx_smulwb(sx_add(b[0], b[11]), f[0]);
        r = sx_smlawb(r, sx_add(b[1], b[10]), f[1]);
        r = sx_smlawb(r, sx_add(b[2], b[9]), f[2]);
        r = sx_smlawb(r, sx_add(b[3], b[8]), f[3]);
        r = sx_smlawb(r, sx_add(b[4], b[7]), f[4]);
        r = sx_smlawb(r, sx_add(b[5], b[6]), f[5]);
    } else {
        const i32 ind = sx_smulwb(idx & 0xFFFF, c.fracs);
        const i16* p = f + (SX_RS_DOWN_FIR / 2) * ind;
        r = sx_smulwb(b[0], p[0]);
#pragma unroll
        for (int t = 1; t < 6; t++) r = sx_smlawb(r, b[t], p[t]);
        p = f + (SX_RS_DOWN_FIR / 2) * (c.fracs - 1 - ind);
#pragma unroll
        for (int t = 0; t < 6; t++) r = sx_smlawb(r, b[11 - t], p[t]);
    }
    return sx_sat16(sx_rshift_round(r, 6));
}
// private_IIR_FIR.c:46-57
SX_HD i32 sx_rs_up_fir(const i16* mid, int j, const SxRsCfg& c) {
    const i32 idx = j * c.inc_Q16;
    const i32 ti = sx_smulwb(idx & 0xFFFF, 144);
    const i16* b = mid + (idx >> 16);
    const i16* f0 = T_rs_frac144 + 3 * ti;
    const i16* f1 = T_rs_frac144 + 3 * (143 - ti);
    i32 r = sx_smulbb(b[0], f0[0]);
    r = sx_smlabb(r, b[1], f0[1]);
    r = sx_smlabb(r, b[2], f0[2]);
    r = sx_smlabb(r, b[3], f1[2]);
    r = sx_smlabb(r, b[4], f1[1]);
    r = sx_smlabb(r, b[5], f1[0]);
    return sx_sat16(sx_rshift_round(r, 15));
}

// ---- a group of up to SX_RS_ROWS rows: what one wavefront does.  lds: SX_RS_ROWS x c.row_words words ---------------------------------
SX_HD void sx_rs_group(const SxRsArgs& a, int row0, u32* lds) {
    const SxRsCfg& c = a.c;
    const int R = sx_min(SX_RS_ROWS, a.n - row0);
    const int W = c.row_words, MW = c.mid_words;
    const int hist = c.kind == 0 ? SX_RS_DOWN_FIR : (c.kind == 1 ? 0 : SX_RS_UP_HIST / 2);      // words of history in sFIR
    const int in_ch = c.n_in >> 3, out_ch = c.n_out >> 3;                                       // 16-byte chunks of a batch
    const size_t in_row = (size_t)a.batches * (size_t)in_ch, out_row = (size_t)a.batches * (size_t)out_ch;
    const SxRsX8* gin = (const SxRsX8*)a.in + (size_t)row0 * in_row;
    SxRsX8* gout = (SxRsX8*)a.out + (size_t)row0 * out_row;
    const i16* coefs = c.coefs == 0 ? T_rs_down_1_3 : (c.coefs == 1 ? T_rs_down_2_3 : T_rs_down_1_2);

    // the state records: sIIR into the recurrence lanes' registers (the 1-lane form walks the rows one after the other and keeps
    // sIIR in the record between batches), the history to the front of the mid buffers
    i32 S[6] = {0, 0, 0, 0, 0, 0};
#if SX_NLANES > 1
    for (int r = SX_LANE; r < R; r += SX_NLANES) {
        const i32* st = a.state + (size_t)(a.map ? a.map[row0 + r] : row0 + r) * SX_RS_STATE_WORDS;
#pragma unroll
        for (int t = 0; t < 6; t++) S[t] = st[t];
    }
#endif
    SX_PAR(i, R * hist) {
        const int r = i / hist, t = i - r * hist;
        lds[r * W + t] = (u32)a.state[(size_t)(a.map ? a.map[row0 + r] : row0 + r) * SX_RS_STATE_WORDS + 6 + t];
    }

    for (int b = 0; b < a.batches; b++) {
        // A: the batch of every row into its staging area
        SX_PAR(i, R * in_ch) {
            const int r = i / in_ch, k = i - r * in_ch;
            const SxRsX8 v = gin[(size_t)r * in_row + (size_t)b * in_ch + k];
            u32* d = lds + r * W + MW + 4 * k;
            d[0] = v.w[0]; d[1] = v.w[1]; d[2] = v.w[2]; d[3] = v.w[3];
        }
        wv_sync();
        // B: one lane per row
        for (int r = SX_LANE; r < R; r += SX_NLANES) {
#if SX_NLANES == 1
            i32* st = a.state + (size_t)(a.map ? a.map[row0 + r] : row0 + r) * SX_RS_STATE_WORDS;
            for (int t = 0; t < 6; t++) S[t] = st[t];
#endif
            u32* mid = lds + r * W;
            const u32* in = mid + MW;
            if (c.kind == 0) sx_rs_ar2(S, in, (i32*)mid, c.n_in, coefs);
            else if (c.kind == 3) sx_rs_up2_lq(S, in, mid, c.n_in);
            else sx_rs_up2_hq(S, in, mid, c.n_in);
#if SX_NLANES == 1
            for (int t = 0; t < 6; t++) st[t] = S[t];
#endif
        }
        wv_sync();
        // C: one output sample per lane and step, into the staging area
        for (int i = SX_LANE, r = 0, j = SX_LANE; i < R * c.n_out; i += SX_NLANES, j += SX_NLANES) {
            while (j >= c.n_out) { j -= c.n_out; r++; }
            const u32* mid = lds + r * W;
            i32 v;
            if (c.kind == 0) v = sx_rs_down_fir((const i32*)mid, j, c, coefs);
            else if (c.kind == 1) v = ((const i16*)mid)[SX_RS_UP_HIST + j];
            else v = sx_rs_up_fir((const i16*)mid, j, c);
            ((i16*)(lds + r * W + MW))[j] = (i16)v;
        }
        wv_sync();
        // D: the staging area to memory; the history to the front (kind 0: words n_in .. n_in + 12, kinds 2, 3: int16 2 n_in .. 2 n_in + 6)
        SX_PAR(i, R * out_ch) {
            const int r = i / out_ch, k = i - r * out_ch;
            const u32* s = lds + r * W + MW + 4 * k;
            SxRsX8 v;
            v.w[0] = s[0]; v.w[1] = s[1]; v.w[2] = s[2]; v.w[3] = s[3];
            gout[(size_t)r * out_row + (size_t)b * out_ch + k] = v;
        }
        SX_PAR(i, R * hist) {
            const int r = i / hist, t = i - r * hist;
            lds[r * W + t] = lds[r * W + c.n_in + t];
        }
        wv_sync();
    }

    // the state records back
#if SX_NLANES > 1
    for (int r = SX_LANE; r < R; r += SX_NLANES) {
        i32* st = a.state + (size_t)(a.map ? a.map[row0 + r] : row0 + r) * SX_RS_STATE_WORDS;
        const int live = c.kind == 0 || c.kind == 3 ? 2 : 6;
#pragma unroll
        for (int t = 0; t < 6; t++) if (t < live) st[t] = S[t];
    }
#endif
    SX_PAR(i, R * hist) {
        const int r = i / hist, t = i - r * hist;
        a.state[(size_t)(a.map ? a.map[row0 + r] : row0 + r) * SX_RS_STATE_WORDS + 6 + t] = (i32)lds[r * W + t];
    }
}

#if defined(__HIPCC__)
extern __shared__ u32 sx_rs_lds[];
// one wavefront per SX_RS_ROWS rows of the call
__global__ void __launch_bounds__(64) solo_resample_kernel(const SxRsArgs a, SxRsCount* count, const u32* verdict) {
    if (sx_map_refused(a.map, verdict)) {
        if (blockIdx.x == 0 && threadIdx.x == 0 && count) count->rows = -1;
        return;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && count) { count->rows = a.n; count->listed = a.n; }
    sx_rs_group(a, (int)blockIdx.x * SX_RS_ROWS, sx_rs_lds);
}
static inline hipError_t solo_resample_launch(const SxRsArgs& a, SxRsCount* count, const u32* verdict, hipStream_t s) {
    const unsigned groups = (unsigned)((a.n + SX_RS_ROWS - 1) / SX_RS_ROWS);
    const size_t lds = (size_t)SX_RS_ROWS * (size_t)a.c.row_words * sizeof(u32);
    hipLaunchKernelGGL(solo_resample_kernel, dim3(groups), dim3(64), lds, s, a, count, verdict);
    return hipGetLastError();
}
#else
// Host form of the launch (tests): every group through sx_rs_group.  -> false: the list is not strictly increasing inside [0, n_rows),
// nothing but count->rows = -1 is written
static inline bool sx_rs_host(const SxRsArgs& a, int n_rows, SxRsCount* count) {
    if (!sx_map_ok(a.map, a.n, n_rows)) {
        if (count) count->rows = -1;
        return false;
    }
    u32* lds = new u32[(size_t)SX_RS_ROWS * (size_t)a.c.row_words]();
    for (int row0 = 0; row0 < a.n; row0 += SX_RS_ROWS) sx_rs_group(a, row0, lds);
    if (count) { count->rows = a.n; count->listed = a.n; }
    delete[] lds;
    return true;
}
#endif

// solo_vad.h -- voice activity, audio level and speaker selection for decoded rows (solo_vad, solo_vad_select, include/solo_mi355x.h).
//
// solo_vad is the reference's fixed-point VAD (SKP_Silk_VAD_Init / SKP_Silk_VAD_GetSA_Q8 with SKP_Silk_VAD_GetNoiseLevels,
// JC1_SDK_SRC_ARM/src/libSATECodec/SKP_Silk_VAD.c:39-318), bit for bit and with its state, as a stage of its own: the encoder runs the
// same arithmetic inside sx_vad (solo_enc_front.h) on the signal it is about to encode, this one runs it on any PCM row, frame by frame,
// for a frame of 160 or 320 samples.  With it comes the RFC 6464 level of every packet:
//
//     E     = sum x^2 over the packet                              64 bits, exact
//     level = the smallest k in [0, 127] with E * 2^20 >= packet_samples * T_k, T_k = round(2^50 * 10^(-k / 10)); none: 127
//
// (x / 32768 is the sample relative to overload, so E / (packet_samples 2^30) >= 10^(-k / 10) is "at or above -k dBov"; with
// packet_samples <= 1920 both sides stay below 2^61.)
//
// The state record of a row is 128 bytes: [0, 112) the reference's SKP_Silk_VAD_state in its own layout (SxVAD of solo_enc_state.h;
// HPstate is an int16 followed by two zero bytes), [112, 128) the selection state {talking, hang, picked, 0} of solo_vad_select.
//
// The analysis kernel: ONE wavefront per row, the row's frames in sequence.  A frame is three all-pass filter banks one behind the
// other (N / 2, N / 4 and N / 8 steps of a two-lane serial recursion: sx_allpass2_chain) and a few hundred instructions of band
// statistics; the frame, the chains' inputs / outputs and the four bands live in LDS (SxVadfLds: 3952 bytes at N = 320, 2080 at N = 160).  The chains are
// what bounds it: 280 dependent steps a frame at N = 320, which no amount of lanes shortens -- only more rows in flight hide them.
//
// solo_vad_select: one wavefront per room, the packets in sequence, per packet one pass over the room's members (thresholds, hangover,
// key) and max_speakers rounds of a wave-wide arg-best over the keys (sx_mix_select, solo_mix.h, whose room plan -- clear,
// check, scan, scatter -- is reused as it is).
//
// Everything outside the kernels compiles for the host with the 1-lane forms of solo_wave.h (tests/test_vad_model.py builds
// sx_vad_host / sx_vsel_host through tests/vad_host.cpp and compares them with the fixture recorded from the compiled reference and with
// the independent model of tests/vad_model.py).
#pragma once
#include <stddef.h>
#include "solo_enc_front.h"     // sx_allpass2_spread / _chain, sx_vad_bank_finish, sx_ana_filt_bank_1, SxVAD
#include "solo_mix.h"           // the room plan, wv_mix_best
#include "solo_vad_tables.inc"

#define SX_VAD_STATE_WORDS 32                               // 28 words of SxVAD | talking, hang, picked, 0
#define SX_VAD_REF_WORDS 28
#define SX_VAD_MAX_PACKET 1920
#define SX_VAD_MAX_SPEAKERS 64
#define SX_VAD_MAX_HANG 1000
#define SX_VAD_MAX_STICK 127

struct SxVadRow { SxVAD v; i32 talking, hang, picked, zero; };
static_assert(sizeof(SxVAD) == SX_VAD_REF_WORDS * 4 && sizeof(SxVadRow) == SX_VAD_STATE_WORDS * 4, "the state record of a row");
typedef solo_vad_count_t SxVadCount;
static_assert(sizeof(SxVadCount) == sizeof(SxMixCount), "the room plan's scan kernel writes {rows, rooms, 0, 0} through a SxMixCount");
typedef solo_vad_select_params_t SxVadSelectParams;

// word w of the record SKP_Silk_VAD_Init leaves (VAD.c:39-67), selection state zero: what the create and reset calls write
SX_HD i32 sx_vad_init_word(int w) {
    if (w >= 10 && w < 14) return 100 * 256;                                    // NrgRatioSmth_Q8: 20 dB
    if (w >= 15 && w < 27) {
        const int b = (w - 15) & 3;
        const i32 bias = sx_max(50 / (b + 1), 1);                               // NoiseLevelBias: approx pink noise
        if (w >= 23) return bias;
        return w >= 19 ? SX_I32_MAX / (100 * bias) : 100 * bias;                // inv_NL, NL
    }
    return w == 27 ? 15 : 0;                                                    // counter
}

static inline bool sx_vad_frame_ok(i32 frame) { return frame == 160 || frame == 320; }
// what the host checks of a solo_vad call before it enqueues anything (rows / count: the call's d_rows and d_count)
static inline bool sx_vad_call_ok(i32 frame, i32 n_rows, const void* rows, i32 n, const void* pcm, i32 n_packets, i32 packet_samples, const void* sa,
                                  const void* count) {
    if (!sx_vad_frame_ok(frame) || !pcm || !sa || (rows && !count) || n <= 0 || n > n_rows || n_packets <= 0) return false;
    if (packet_samples <= 0 || packet_samples > SX_VAD_MAX_PACKET || packet_samples % frame) return false;
    const i64 np = (i64)n * (i64)n_packets;
    if (np * packet_samples >= ((i64)1 << 31) || np * (packet_samples / frame) * 6 >= ((i64)1 << 31)) return false;
    return !((uintptr_t)pcm & 15);
}
static inline bool sx_vsel_params_ok(const SxVadSelectParams* p) {
    return p && p->max_speakers >= 1 && p->max_speakers <= SX_VAD_MAX_SPEAKERS && p->off_q8 >= 0 && p->off_q8 <= p->on_q8 && p->on_q8 <= 255 &&
           p->hang_packets >= 0 && p->hang_packets <= SX_VAD_MAX_HANG && p->stick >= 0 && p->stick <= SX_VAD_MAX_STICK;
}
// ... of a solo_vad_select call
static inline bool sx_vsel_call_ok(i32 n_rows, i32 n, const void* sa, const void* level, i32 n_packets, i32 frames, const void* room, i32 n_rooms,
                                   const SxVadSelectParams* p, const void* sel, const void* count) {
    if (!sa || !level || !room || !sel || !count || !sx_vsel_params_ok(p)) return false;
    if (n <= 0 || n > n_rows || n_packets <= 0 || frames <= 0 || n_rooms <= 0 || n_rooms > n_rows) return false;
    return (i64)n * (i64)n_packets * (i64)frames < ((i64)1 << 31) && (i64)n_rooms * (i64)n_packets < ((i64)1 << 31);
}
// (the name the host builds of tests/vad_host.cpp and tests/agc_host.cpp ask the host-list rule by)
static inline bool sx_vad_list_ok(const i32* rows, i32 n, i32 n_rows) { return sx_list_ok(rows, n, n_rows); }

// ---- one frame of N samples ---------------------------------------------------------------------------------------------------------
// LDS of a row (the host form: plain memory).  X holds the bands, highest first: X3 (N / 2 samples), X2 (N / 4), X1 (N / 8), X0 (N / 8,
// and room for the N / 2 samples the serial host form of the first bank leaves there).
template <int N>
struct alignas(16) SxVadfLds {
    i32 raw[N + N / 2 + N / 4];         // the chain inputs / outputs of the three banks
    i16 pcm[N];
    i16 X[7 * N / 8 + N / 2];
    i32 part[16];
    SxVadRow st;
};
struct SxVadfOut { i32 sa_Q8, snr_dB_Q7, tilt_Q15; };      // (Quality_Q15[b]: part[4 * b + 1] of the row's LDS)

// SKP_Silk_VAD_GetSA_Q8 (VAD.c:75-255) with SKP_Silk_VAD_GetNoiseLevels (VAD.c:260-318) on L->pcm, state L->st.v
template <int N>
SX_HD SxVadfOut sx_vadf_frame(SxVadfLds<N>* L) {
    static_assert(N == 160 || N == 320, "a frame of 160 or 320 samples");
    SX_IN_LDS(L);
    SxVAD* v = &L->st.v;
    i16* const X3 = L->X, * const X2 = X3 + N / 2, * const X1 = X2 + N / 4, * const X0 = X1 + N / 8;
    i32* const part = L->part;
#ifdef SX_LANE_STREAM
    {
        // the three banks one after the other, every bank's low band going straight from its finish pass into the next bank's chain inputs
        constexpr int h1 = N / 2, h2 = N / 4, h3 = N / 8;
        i32* a1 = L->raw, *a2 = a1 + 2 * h1, *a3 = a2 + 2 * h2;
        sx_allpass2_spread<N>(L->pcm, a1, h1);
        wv_sync();
        sx_allpass2_chain<h1>(a1, h1, v->AnaState, SX_A_FB1_21, SX_A_FB1_20);
        sx_vad_bank_finish<h1, false>(a1, X3, (i16*)0, a2);
        sx_allpass2_chain<h2>(a2, h2, v->AnaState1, SX_A_FB1_21, SX_A_FB1_20);
        sx_vad_bank_finish<h2, false>(a2, X2, (i16*)0, a3);
        sx_allpass2_chain<h3>(a3, h3, v->AnaState2, SX_A_FB1_21, SX_A_FB1_20);
        sx_vad_bank_finish<h3, true>(a3, X1, X0, (i32*)0);
    }
#else
    sx_ana_filt_bank_1(L->pcm, v->AnaState, X0, X3, N);
    sx_ana_filt_bank_1(X0, v->AnaState1, X0, X2, N >> 1);
    sx_ana_filt_bank_1(X0, v->AnaState2, X0, X1, N >> 2);
#endif
    // HP filter on the lowest band (differentiator): h[i] = X0[i] >> 1, X0[i] = h[i] - h[i - 1] (h[-1] = the state), state = h[last]
    constexpr int dfl = N >> 3;
    static_assert(dfl <= 64, "one sample of the lowest band per lane");
    {
        i16 hs[(dfl + SX_NLANES - 1) / SX_NLANES], hm[(dfl + SX_NLANES - 1) / SX_NLANES];
        const i16 hp = (i16)v->HPstate;
        int t = 0;
        SX_PAR(i, dfl) { hs[t] = (i16)(X0[i] >> 1); hm[t] = i > 0 ? (i16)(X0[i - 1] >> 1) : hp; t++; }
        wv_sync();
        t = 0;
        SX_PAR(i, dfl) {
            X0[i] = (i16)(hs[t] - hm[t]);
            if (i == dfl - 1) v->HPstate = (i32)(u16)hs[t];
            t++;
        }
        wv_sync();
    }
    // band energies: lane (b, q) sums the squares of quarter q of band b ...
    SX_PAR(t, 16) {
        const int b = t >> 2, q = t & 3;
        const int sub_len = (N >> sx_min(4 - b, 3)) >> 2;
        const i16* Xb = (b == 0 ? X0 : (b == 1 ? X1 : (b == 2 ? X2 : X3))) + q * sub_len;
        i32 sum = 0;
        for (int i = 0; i < sub_len; i++) {
            const i32 x_tmp = Xb[i] >> 3;
            sum = sx_smlabb(sum, x_tmp, x_tmp);
        }
        part[t] = sum;
    }
    wv_sync();
    // ... and lane b folds its band's four with the reference's saturating adds, then runs the band's noise-level tracker and
    // signal-to-noise terms; the sums over the bands are wrapping adds of per-band terms
    const i32 min_coef = v->counter < 1000 ? 32767 / ((v->counter >> 4) + 1) : 0;
    wv_sync();
    SX_PAR(b, 4) {
        i32 e = v->XnrgSubfr[b];
        for (int q = 0; q < 3; q++) e = sx_add_pos_sat32(e, part[4 * b + q]);
        const i32 last = part[4 * b + 3];
        e = sx_add_pos_sat32(e, last >> 1);
        v->XnrgSubfr[b] = last;
        i32 nl = v->NL[b];
        {
            const i32 nrg = sx_add_pos_sat32(e, v->NoiseLevelBias[b]);
            const i32 inv_nrg = SX_I32_MAX / nrg;
            i32 coef;
            if (nrg > sx_shl(nl, 3)) coef = 1024 >> 3;
            else if (nrg < nl) coef = 1024;
            else coef = sx_smulwb(sx_smulww(inv_nrg, nl), 1024 << 1);
            coef = sx_max(coef, min_coef);
            v->inv_NL[b] = sx_smlawb(v->inv_NL[b], inv_nrg - v->inv_NL[b], coef);
            nl = SX_I32_MAX / v->inv_NL[b];
            nl = sx_min(nl, 0x00FFFFFF);
            v->NL[b] = nl;
        }
        i32 ratio = 256, sq = 0, tilt = 0;
        const i32 speech_nrg_b = e - nl;
        if (speech_nrg_b > 0) {
            if ((e & 0xFF800000) == 0) ratio = sx_shl(e, 8) / (nl + 1);
            else ratio = e / ((nl >> 8) + 1);
            i32 SNR_Q7 = sx_lin2log(ratio) - 8 * 128;
            sq = sx_smulbb(SNR_Q7, SNR_Q7);
            if (speech_nrg_b < (1 << 20)) SNR_Q7 = sx_smulwb(sx_shl(sx_sqrt_approx(speech_nrg_b), 6), SNR_Q7);
            tilt = sx_smulwb(T_vad_tilt_weights[b], SNR_Q7);
        }
        part[4 * b] = ratio; part[4 * b + 1] = sq; part[4 * b + 2] = tilt; part[4 * b + 3] = (b + 1) * (speech_nrg_b >> 4);
        if (b == 0) v->counter++;
    }
    wv_sync();
    i32 sumSquared = 0, input_tilt = 0, speech_nrg = 0;
    for (int b = 0; b < 4; b++) {
        sumSquared = sx_add(sumSquared, part[4 * b + 1]);
        input_tilt = sx_add(input_tilt, part[4 * b + 2]);
        speech_nrg = sx_add(speech_nrg, part[4 * b + 3]);
    }
    wv_sync();
    SxVadfOut o;
    sumSquared = sumSquared / 4;
    o.snr_dB_Q7 = (i16)(3 * sx_sqrt_approx(sumSquared));
    i32 SA_Q15 = sx_sigm_Q15(sx_smulwb(45000, o.snr_dB_Q7) - 128);
    o.tilt_Q15 = sx_shl(sx_sigm_Q15(input_tilt) - 16384, 1);
    if (speech_nrg <= 0) {
        SA_Q15 = SA_Q15 >> 1;
    } else if (speech_nrg < 32768) {
        speech_nrg = sx_sqrt_approx(sx_shl(speech_nrg, 15));
        SA_Q15 = sx_smulwb(32768 + speech_nrg, SA_Q15);
    }
    o.sa_Q8 = sx_min(SA_Q15 >> 7, 255);
    const i32 smooth_coef_Q16 = (i16)sx_smulwb(4096, sx_smulwb(SA_Q15, SA_Q15));
    SX_PAR(b, 4) {
        v->NrgRatioSmth_Q8[b] = sx_smlawb(v->NrgRatioSmth_Q8[b], part[4 * b] - v->NrgRatioSmth_Q8[b], smooth_coef_Q16);
        const i32 SNR_Q7 = 3 * (sx_lin2log(v->NrgRatioSmth_Q8[b]) - 8 * 128);
        part[4 * b + 1] = sx_sigm_Q15((SNR_Q7 - 16 * 128) >> 4);
    }
    wv_sync();
    return o;
}

// the RFC 6464 level of a packet of Ls samples with energy E (wave-uniform)
SX_HD i32 sx_vad_level(i64 E, i32 Ls) {
    const u64 lhs = (u64)E << 20;
    i32 best = 127;
    SX_PAR(k, 128) if (lhs >= (u64)Ls * T_vad_level[k]) best = sx_min(best, k);
    return wv_min(best);
}

struct alignas(16) SxVadX8 { i16 s[8]; };                  // what one lane loads: 8 samples

struct SxVadArgs {
    const i16* pcm;                 // [n][P][Ls]
    i32* state;                     // [n_rows][SX_VAD_STATE_WORDS]
    const i32* map;                 // compact position -> row of the object, or NULL = the identity
    u8* sa; i32* detail; u8* level; // [n][P][F], [n][P][F][6] or NULL, [n][P] or NULL
    i32 n, n_packets, packet_samples;
};

// row i of a call: what one wavefront does
template <int N>
SX_HD void sx_vadf_row(const SxVadArgs& a, int i, SxVadfLds<N>* L) {
    const int P = a.n_packets, Ls = a.packet_samples, F = Ls / N;
    i32* const g = a.state + (size_t)(a.map ? SX_UNI(a.map[i]) : i) * SX_VAD_STATE_WORDS;
    i32* const st = (i32*)&L->st;
    SX_PAR(w, SX_VAD_REF_WORDS) st[w] = g[w];
    wv_sync();
    const SxVadX8* row = (const SxVadX8*)(a.pcm + (size_t)i * (size_t)P * (size_t)Ls);
    for (int p = 0; p < P; p++) {
        i64 e = 0;
        for (int f = 0; f < F; f++) {
            SX_PAR(k, N / 8) {
                const SxVadX8 x = row[((size_t)p * F + f) * (N / 8) + k];
#pragma unroll
                for (int s = 0; s < 8; s++) { L->pcm[8 * k + s] = x.s[s]; e += (i64)((i32)x.s[s] * (i32)x.s[s]); }
            }
            wv_sync();
            const SxVadfOut o = sx_vadf_frame<N>(L);
            const size_t at = ((size_t)i * P + p) * F + f;
            if (SX_LANE == 0) a.sa[at] = (u8)o.sa_Q8;
            if (a.detail) {
                if (SX_LANE == 0) { a.detail[at * 6] = o.snr_dB_Q7; a.detail[at * 6 + 1] = o.tilt_Q15; }
                SX_PAR(b, 4) a.detail[at * 6 + 2 + b] = L->part[4 * b + 1];
            }
            wv_sync();
        }
        if (a.level) {
            const i32 lv = sx_vad_level(wv_sum64(e), Ls);
            if (SX_LANE == 0) a.level[(size_t)i * P + p] = (u8)lv;
        }
    }
    SX_PAR(w, SX_VAD_REF_WORDS) g[w] = st[w];
}

// ---- the selection: one room, its packets in sequence ---------------------------------------------------------------------------------
struct SxVselArgs {
    const u8* sa; const u8* level;  // [n][P][F], [n][P]
    const i16* gain_in;             // [n] or NULL = 4096
    const i32* map;                 // compact position -> row of the object, or NULL
    u8* sel; i16* gain_out; u8* keep; i32* dominant;        // [n][P], [n] or NULL, [n] or NULL, [n_rooms][P] or NULL
    i32* state;                     // [n_rows][SX_VAD_STATE_WORDS]
    i32* key;                       // scratch [n]: the packet's keys
    const i32* counts; const i32* starts; const i32* members;       // the room plan (solo_mix.h)
    i32 n_packets, frames;
    SxVadSelectParams prm;
};
SX_HD i32* sx_vsel_state(const SxVselArgs& a, i32 i) { return a.state + (size_t)(a.map ? a.map[i] : i) * SX_VAD_STATE_WORDS + SX_VAD_REF_WORDS; }

// The keys of a packet are kept as ONE word: 2 * key + s for a candidate (larger first = larger key first, then the incumbent), -1 - s
// for a row that is none (never selected; s travels along for the count of changes).  Equal words: the smaller row position first --
// the order of sx_mix_before.  -> selected (row, packet) pairs and changes of s of the room, in every lane
SX_HD void sx_vsel_room(const SxVselArgs& a, int room, i32* n_selected, i32* n_changes) {
    const int m = SX_UNI(a.counts[room]);
    const int P = a.n_packets, F = a.frames;
    i32 selected = 0, changes = 0;
    *n_selected = 0; *n_changes = 0;
    if (m <= 0) {
        if (a.dominant) SX_PAR(p, P) a.dominant[(size_t)room * P + p] = -1;
        return;
    }
    const i32* mem = a.members + SX_UNI(a.starts[room]);
    const int K = sx_min(a.prm.max_speakers, m);
    for (int p = 0; p < P; p++) {
        i32 old_on = 0;
        for (int j = SX_LANE; j < m; j += SX_NLANES) {
            const i32 i = mem[j];
            i32* st = sx_vsel_state(a, i);
            i32 t = st[0], h = st[1];
            const i32 s = st[2] != 0;
            const u8* fr = a.sa + ((size_t)i * P + p) * F;
            i32 act = 0;
            for (int f = 0; f < F; f++) act = sx_max(act, (i32)fr[f]);
            bool cand;
            if (act >= (t ? a.prm.off_q8 : a.prm.on_q8)) { t = 1; h = a.prm.hang_packets; cand = true; }
            else { t = 0; cand = h > 0; h = sx_max(h - 1, 0); }
            st[0] = t; st[1] = h; st[2] = 0;
            a.sel[(size_t)i * P + p] = 0;
            const i32 lv = sx_min((i32)a.level[(size_t)i * P + p], 127);
            a.key[i] = cand ? 2 * ((127 - lv) + (s ? a.prm.stick : 0)) + s : -1 - s;
            old_on += s;
        }
        old_on = wv_sum(old_on);
        wv_sync();
        // round k picks the first candidate that comes after pick k - 1 (fewer candidates than max_speakers: fewer picks)
        i32 first = -1, picked_old = 0;
        const i32 npick = sx_mix_select(mem, m, K, [&](i32 row) { const i32 e = a.key[row]; return (i64)(e < 0 ? -2 : e); },
                                        [&](int k, i32 row, i64 key) {
                                            if (SX_LANE == 0) { sx_vsel_state(a, row)[2] = 1; a.sel[(size_t)row * P + p] = 1; }
                                            if (k == 0) first = row;
                                            picked_old += (i32)(key & 1);
                                        });
        if (a.dominant && SX_LANE == 0) a.dominant[(size_t)room * P + p] = first;
        selected += npick;
        changes += (npick - picked_old) + (old_on - picked_old);    // newcomers, and incumbents that were not picked again
        wv_sync();
    }
    // after the last packet: the gains and the hangover flags a mix takes
    for (int j = SX_LANE; j < m; j += SX_NLANES) {
        const i32 i = mem[j];
        if (a.gain_out) a.gain_out[i] = sx_vsel_state(a, i)[2] ? (i16)sx_mix_gain(a.gain_in, i) : (i16)0;
        if (a.keep) a.keep[i] = a.key[i] >= 0;
    }
    *n_selected = selected; *n_changes = changes;
}

// bytes of device scratch of an object of n_rows rows (rooms <= n_rows): the room plan (solo_mix.h) | key
static inline size_t solo_vad_scratch_bytes(int n_rows) { return sx_room_plan_bytes(n_rows) + (size_t)n_rows * sizeof(i32); }

#if defined(__HIPCC__)
// one wavefront per row of the call
template <int N>
__global__ void __launch_bounds__(64) solo_vad_kernel(const SxVadArgs a, SxVadCount* count, const u32* verdict) {
    __shared__ SxVadfLds<N> lds;
    if (sx_map_refused(a.map, verdict)) {
        if (blockIdx.x == 0 && threadIdx.x == 0 && count) count->rows = -1;
        return;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && count) { SxVadCount c; c.rows = a.n; c.rooms = 0; c.selected = 0; c.changes = 0; *count = c; }
    sx_vadf_row<N>(a, (int)blockIdx.x, &lds);
}
// one wavefront per room
__global__ void __launch_bounds__(64) solo_vad_select_kernel(const SxVselArgs a, SxVadCount* count, const i32* room_ids, const u32* verdict) {
    if (sx_map_refused(room_ids, verdict)) return;
    i32 selected, changes;
    sx_vsel_room(a, (int)blockIdx.x, &selected, &changes);
    if (threadIdx.x == 0 && selected) atomicAdd(&count->selected, selected);
    if (threadIdx.x == 0 && changes) atomicAdd(&count->changes, changes);
}

static inline hipError_t solo_vad_launch(int frame, const SxVadArgs& a, SxVadCount* count, const u32* verdict, hipStream_t s) {
    if (frame == 320) hipLaunchKernelGGL(solo_vad_kernel<320>, dim3((unsigned)a.n), dim3(64), 0, s, a, count, verdict);
    else hipLaunchKernelGGL(solo_vad_kernel<160>, dim3((unsigned)a.n), dim3(64), 0, s, a, count, verdict);
    return hipGetLastError();
}
// scratch: solo_vad_scratch_bytes(n_rows) bytes.  The verdict word is cleared by the plan, set by the list check that the caller enqueues
// between the clear and the rest (list_check(verdict), or nothing), and by the room ids' check
template <typename ListCheck>
static inline hipError_t solo_vad_select_launch(SxVselArgs a, const i32* room, int n, int n_rooms, int n_rows, void* scratch, SxVadCount* count, u32* verdict,
                                                ListCheck list_check, hipStream_t s) {
    const SxRoomPlan rp = sx_room_plan(scratch, n_rows);
    a.key = sx_room_plan_end(rp, n_rows); a.counts = rp.counts; a.starts = rp.starts; a.members = rp.members;
    sx_room_plan_launch(rp, room, n, n_rooms, (SxMixCount*)count, verdict, list_check, s);
    hipLaunchKernelGGL(solo_vad_select_kernel, dim3((unsigned)n_rooms), dim3(64), 0, s, a, count, room, verdict);
    return hipGetLastError();
}
#else
// Host form of the launch (tests): every row through sx_vadf_row.  -> false: the list is not strictly increasing inside [0, n_rows),
// nothing but count->rows = -1 is written
template <int N>
static inline bool sx_vad_host_n(const SxVadArgs& a, int n_rows, SxVadCount* count) {
    if (!sx_map_ok(a.map, a.n, n_rows)) {
        if (count) count->rows = -1;
        return false;
    }
    SxVadfLds<N>* L = new SxVadfLds<N>();
    for (int i = 0; i < a.n; i++) sx_vadf_row<N>(a, i, L);
    delete L;
    if (count) { count->rows = a.n; count->rooms = 0; count->selected = 0; count->changes = 0; }
    return true;
}
static inline bool sx_vad_host(int frame, const SxVadArgs& a, int n_rows, SxVadCount* count) {
    return frame == 320 ? sx_vad_host_n<320>(a, n_rows, count) : sx_vad_host_n<160>(a, n_rows, count);
}
// ... of the selection: the room plan (sx_room_plan_host), then every room through sx_vsel_room.
// -> false: a bad list or a room id outside [-1, n_rooms), nothing but count->rows = -1 is written
static inline bool sx_vsel_host(SxVselArgs a, const i32* room, int n, int n_rooms, int n_rows, SxVadCount* count) {
    bool ok = sx_map_ok(a.map, n, n_rows);
    for (int i = 0; ok && i < n; i++) ok = room[i] >= -1 && room[i] < n_rooms;
    if (!ok) {
        count->rows = -1;
        return false;
    }
    const int cap = sx_max(sx_max(n, n_rooms), n_rows);
    i32* words = new i32[solo_vad_scratch_bytes(cap) / sizeof(i32)]();
    const SxRoomPlan rp = sx_room_plan(words, cap);
    SxVadCount c; c.selected = 0; c.changes = 0;
    sx_room_plan_host(rp, room, n, n_rooms, &c.rows, &c.rooms);
    a.counts = rp.counts; a.starts = rp.starts; a.members = rp.members; a.key = sx_room_plan_end(rp, cap);
    for (int r = 0; r < n_rooms; r++) {
        i32 s, ch;
        sx_vsel_room(a, r, &s, &ch);
        c.selected += s; c.changes += ch;
    }
    *count = c;
    delete[] words;
    return true;
}
#endif
